"""ctws_block_morphology on the GPU against the CPU restatement (tests/morphology_ref.py): all 11
columns by assert_array_equal -- both sides divide two exactly representable integers -- on the
smallest shapes at which each mechanism of k_morph.hip can fail, the refusals of the documented
limits, the capacity protocol, the device path and byte-for-byte repeatability."""
import ctypes as C

import numpy as np
import pytest

from cluster_tools_amd import ctws
from cluster_tools_amd.ctws import lib
import morphology_ref as R

pytestmark = pytest.mark.gpu


def _check(h, labels, begin=(0, 0, 0)):
    labels = np.ascontiguousarray(labels, dtype=np.uint64)
    got = h.block_morphology(labels, begin)
    want = R.block_morphology(labels, begin)
    assert got.dtype == np.float64 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    return got


def _coherent(seed, shape, cell, n_ids=40):
    """Fragments: a coarse random grid enlarged to cells, with sprinkled single voxels."""
    rng = np.random.RandomState(seed)
    coarse = rng.randint(0, n_ids, tuple(-(-s // c) for s, c in zip(shape, cell))).astype(np.uint64)
    vol = np.kron(coarse, np.ones(cell, dtype=np.uint64))[tuple(slice(0, s) for s in shape)]
    vol = np.ascontiguousarray(vol)
    vol[rng.rand(*shape) < .01] = n_ids + 1
    return vol


@pytest.mark.parametrize('shape', [
    (1, 1, 1),    # a single voxel
    (3, 5, 7),    # a partial word
    (2, 3, 64),   # exactly one word
    (2, 3, 65),   # a fragment's run crossing a word end
    (1, 2, 129),
])
def test_small_shapes(gpu_handle, shape):
    rng = np.random.RandomState(sum(shape))
    # runs of random lengths along x, so that some cross the word ends at 64 and 128
    lab = np.repeat(rng.randint(0, 4, (shape[0], shape[1], shape[2])), 5, axis=2)[:, :, 2:2 + shape[2]]
    _check(gpu_handle, lab)
    _check(gpu_handle, np.full(shape, 3))


def test_one_id_fills_the_block(gpu_handle):
    got = _check(gpu_handle, np.full((4, 8, 200), 9))  # runs of full length
    assert got.tolist() == [[9, 6400, 1.5, 3.5, 99.5, 0, 0, 0, 3, 7, 199]]
    assert gpu_handle.timings()['morph_run_passes'] == 1.  # a run per row, or per word, fits 1,600


@pytest.mark.parametrize('shape', [(1, 2, 384), (3, 4, 70)])
def test_every_voxel_distinct(gpu_handle, shape):
    """More emits per wave than one LDS stage holds: the flush inside the row loop."""
    n = int(np.prod(shape))
    lab = np.random.RandomState(1).permutation(n).reshape(shape)
    got = _check(gpu_handle, lab)
    assert len(got) == n and (got[:, 1] == 1).all()
    if n > 256:  # more runs than the first buffer of max(64, n / 4) holds
        assert gpu_handle.timings()['morph_run_passes'] == 2.
    np.testing.assert_array_equal(got[:, 2:5], got[:, 5:8])


def test_high_id_bits(gpu_handle):
    """The sort's high bits; 0 is counted like any other id."""
    ids = np.array([0, 1, 2 ** 32 + 1, 2 ** 40, 2 ** 53 - 1], dtype=np.uint64)
    lab = ids[np.random.RandomState(2).randint(0, len(ids), (3, 6, 70))]
    got = _check(gpu_handle, lab)
    assert got[:, 0].tolist() == [float(i) for i in ids] and got[0, 1] > 0
    assert int(got[-1, 0]) == 2 ** 53 - 1


def test_global_coordinates(gpu_handle):
    begin = (1000, 2 ** 20, 7)
    got = _check(gpu_handle, _coherent(3, (5, 9, 70), (2, 4, 16)), begin)
    assert (got[:, 5:8] >= np.array(begin)).all() and got[:, 3].min() >= 2 ** 20


def test_coherent_random_block(gpu_handle):
    lab = _coherent(4, (12, 40, 200), (5, 9, 37))
    got = _check(gpu_handle, lab)
    assert len(got) > 30 and got[:, 1].sum() == lab.size


@pytest.mark.parametrize('front', [0, 1, 700, 2048])
def test_long_segments_are_split(gpu_handle, front):
    """Ids that own more than two chunks of 2048 sorted records: the aligned chunks inside their
    segments go to waves of their own and meet the head and tail in the per-id table.  `front`
    records of a smaller id put the segments' first records on, one past and between the chunk
    borders; front = 0 and 2048 leave a segment without a head."""
    lab = np.empty((4, 16, 200), dtype=np.uint64)
    lab[:, :, 0::2] = 5  # alternating voxels: 6400 runs of length 1 each
    lab[:, :, 1::2] = 2 ** 40 + 7
    flat = lab.reshape(-1)
    flat[1:2 * front:2] = 3  # `front` records of id 3, taken from the second id
    got = _check(gpu_handle, lab, (3, 2, 1))
    assert got[:, 0].tolist() == ([3.] if front else []) + [5., float(2 ** 40 + 7)]
    assert got[-2, 1] == 6400 and got[-1, 1] == 6400 - front
    a = gpu_handle.block_morphology(lab, (3, 2, 1))
    assert a.tobytes() == got.tobytes()


def test_one_long_segment_beside_many_short_ones(gpu_handle):
    """A background id owning most of the records (the case the split was measured for) among
    fragments of a few records each."""
    rng = np.random.RandomState(8)
    lab = np.zeros((6, 30, 130), dtype=np.uint64)
    dots = rng.rand(*lab.shape) < .3
    lab[dots] = rng.randint(1, 400, int(dots.sum()))
    got = _check(gpu_handle, lab, (0, 64, 128))
    assert got[0, 0] == 0 and got[0, 1] > .6 * lab.size and len(got) == 400


def test_all_zero_block_gives_the_row_of_zero(gpu_handle):
    got = _check(gpu_handle, np.zeros((2, 3, 70)), (4, 0, 8))
    assert got.tolist() == [[0, 420, 4.5, 1, 42.5, 4, 0, 8, 5, 2, 77]]


def test_refusals(gpu_handle):
    lab = np.ones((2, 2, 3), dtype=np.uint64)
    lab[1, 1, 2] = 2 ** 53
    with pytest.raises(ctws.CtwsError, match='2\\^53'):
        gpu_handle.block_morphology(lab)
    ret, m, rows = gpu_handle.block_morphology_raw(lab, (0, 0, 0), 8)
    assert ret == -5 and np.isnan(rows).all()  # CTWS_EUNSUPPORTED, nothing written
    lab[1, 1, 2] = 2 ** 53 - 1
    _check(gpu_handle, lab)
    # begin + extent <= 2^21 on every axis
    for axis in range(3):
        begin = [0, 0, 0]
        begin[axis] = 2 ** 21 - lab.shape[axis]
        _check(gpu_handle, lab, begin)
        begin[axis] += 1
        with pytest.raises(ctws.CtwsError, match='2\\^21'):
            gpu_handle.block_morphology(lab, begin)
        ret, m, rows = gpu_handle.block_morphology_raw(lab, begin, 8)
        assert ret == -5 and m == 0 and np.isnan(rows).all()
    with pytest.raises(ctws.CtwsError):
        gpu_handle.block_morphology(lab, (0, -1, 0))
    with pytest.raises(TypeError):
        gpu_handle.block_morphology(lab.astype(np.int64))


def test_capacity(gpu_handle):
    lab = _coherent(5, (4, 10, 70), (2, 3, 11), n_ids=20)
    want = R.block_morphology(lab, (1, 2, 3))
    m = len(want)
    assert m > 10
    ret, got_m, rows = gpu_handle.block_morphology_raw(lab, (1, 2, 3), m - 1)
    assert ret == -1 and got_m == m and np.isnan(rows).all()  # CTWS_EINVAL, n_rows set, nothing written
    assert 'capacity' in lib().ctws_last_error(gpu_handle._h).decode()
    ret, got_m, rows = gpu_handle.block_morphology_raw(lab, (1, 2, 3), m)
    assert ret == 0 and got_m == m
    np.testing.assert_array_equal(rows, want)
    # a zero capacity without a buffer
    n = C.c_int64(-1)
    ret = lib().ctws_block_morphology(gpu_handle._h, lab.ctypes.data, *lab.shape, (C.c_int64 * 3)(0, 0, 0), None, 0,
                                      C.byref(n))
    assert ret == -1 and n.value == m


def test_retry_on_capacity(gpu_handle, monkeypatch):
    lab = _coherent(6, (3, 8, 70), (1, 2, 7), n_ids=30)
    monkeypatch.setattr(ctws.Handle, 'MORPHOLOGY_CAP', 4)
    _check(gpu_handle, lab)
    import torch
    d = gpu_handle.block_morphology_device(torch.from_numpy(lab.view(np.int64)).cuda())
    np.testing.assert_array_equal(d.cpu().numpy(), R.block_morphology(lab))


def test_device_path_and_repeatability(gpu_handle):
    import torch
    lab = _coherent(7, (6, 20, 130), (3, 7, 23))
    begin = (8, 16, 64)
    a = gpu_handle.block_morphology(lab, begin)
    t = dict(gpu_handle.timings())
    for name in ('morph_runs', 'morph_sort', 'morph_rows', 'morph_emits'):
        assert name in t, (name, sorted(t))
    assert lab.size / 64 <= t['morph_emits'] <= lab.size
    b = gpu_handle.block_morphology(lab, begin)
    assert a.tobytes() == b.tobytes()
    d = gpu_handle.block_morphology_device(torch.from_numpy(lab.view(np.int64)).cuda(), begin)
    assert d.is_cuda and d.dtype == torch.float64
    assert d.cpu().numpy().tobytes() == a.tobytes()
    np.testing.assert_array_equal(a, R.block_morphology(lab, begin))
