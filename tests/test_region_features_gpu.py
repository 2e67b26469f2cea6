"""ctws_region_features_block on the GPU against the CPU restatement (tests/region_features_ref.py).
Where the values sum exactly in float64 in any order -- uint8 (v / 255 in float32 is a multiple of
2^-31 and at most 1, so up to 2^21 voxels sum exactly), uint16, floats k / 1024 -- all three
columns by assert_array_equal, on the smallest shapes at which each mechanism of k_regfeat.hip can
fail.  General floats against the exactly rounded sum within the bound of a float64 sum in any
order.  The refusals, the capacity protocol, the device path and byte-for-byte repeatability."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from cluster_tools_amd import ctws
from cluster_tools_amd.ctws import lib
import region_features_ref as R

pytestmark = pytest.mark.gpu

DTYPES = ['uint8', 'uint16', 'float32', 'float64']


def _summable(rng, shape, dtype):
    """Values whose float32 forms sum exactly in float64 in any order."""
    if dtype == 'uint8':
        return rng.randint(0, 256, shape).astype('uint8')
    if dtype == 'uint16':
        return rng.randint(0, 65536, shape).astype('uint16')
    return (rng.randint(0, 1024, shape) / 1024.).astype(dtype)


def _check(h, labels, data, ignore_label=0):
    labels = np.ascontiguousarray(labels, dtype=np.uint64)
    got = h.region_features_block(labels, data, ignore_label)
    want = R.block_rows(labels, data, ignore_label)
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


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [
    (1, 1, 1),    # a single voxel
    (3, 5, 7),    # a partial word
    (2, 3, 64),   # exactly one word
    (2, 3, 65),   # a fragment's run crossing a word end
    (1, 2, 129),
])
def test_small_shapes(gpu_handle, shape, dtype):
    rng = np.random.RandomState(sum(shape))
    # runs of random lengths along x, so that some cross the word ends at 64 and 128
    lab = np.repeat(rng.randint(0, 4, (shape[0], shape[1], shape[2])), 5, axis=2)[:, :, 2:2 + shape[2]]
    data = _summable(rng, shape, dtype)
    for ignore_label in (0, None):
        _check(gpu_handle, lab, data, ignore_label)
    _check(gpu_handle, np.full(shape, 3), data)


def test_one_id_fills_the_block(gpu_handle):
    shape = (4, 8, 200)  # runs of full length
    got = _check(gpu_handle, np.full(shape, 9), np.full(shape, .5, dtype='float32'))
    assert got.tolist() == [[9, 6400, 0.5]]
    got = _check(gpu_handle, np.full(shape, 9), np.full(shape, 255, dtype='uint8'))
    assert got.tolist() == [[9, 6400, 1.0]]


@pytest.mark.parametrize('shape', [(1, 2, 384), (3, 4, 70)])
def test_every_voxel_distinct(gpu_handle, shape):
    n = int(np.prod(shape))
    rng = np.random.RandomState(1)
    lab = rng.permutation(n).reshape(shape) + 1
    data = rng.randn(*shape).astype('float32')
    got = _check(gpu_handle, lab, data)
    assert len(got) == n and (got[:, 1] == 1).all()
    np.testing.assert_array_equal(got[np.argsort(np.argsort(lab.ravel())), 2], data.ravel().astype('float64'))


def test_row_offsets(gpu_handle):
    """Row r holds r % 7 + 1 runs: every record's place comes from the scan of the rows' counts."""
    shape = (3, 9, 130)
    lab = np.zeros(shape, dtype=np.uint64)
    want_records = 0
    for r in range(shape[0] * shape[1]):
        runs = r % 7 + 1
        cuts = np.linspace(0, shape[2], runs + 1).astype(int)
        for k in range(runs):
            lab.reshape(-1, shape[2])[r, cuts[k]:cuts[k + 1]] = 1 + (r * 5 + k * 3) % 23 + (k % 2) * 100
        # (neighbouring runs of a row differ: k % 2 moves every other one by 100)
        want_records += sum(-(-(cuts[k + 1]) // 64) - cuts[k] // 64 for k in range(runs))
    rng = np.random.RandomState(2)
    for dtype in ('float32', 'uint8'):
        _check(gpu_handle, lab, _summable(rng, shape, dtype), None)
    assert dict(gpu_handle.timings())['regfeat_records'] == want_records


def test_dtype_handling(gpu_handle):
    lab = np.array([1, 2, 3, 4], dtype=np.uint64).reshape(1, 1, 4)
    d = np.array([.1, 1 / 3, 1 + 2. ** -30, 1 + 2. ** -24 + 2. ** -40], dtype='float64').reshape(1, 1, 4)
    got = gpu_handle.region_features_block(lab, d)
    # rounded to float32 first, to nearest: the last lies just above a tie and goes up
    assert got[:, 2].tolist() == [float(np.float32(.1)), float(np.float32(1 / 3)), 1.0, 1 + 2. ** -23]
    _check(gpu_handle, lab, d)
    got = _check(gpu_handle, lab, np.array([65535, 0, 1, 256], dtype='uint16').reshape(1, 1, 4))
    assert got[:, 2].tolist() == [65535., 0., 1., 256.]  # uint16 is not scaled
    got = _check(gpu_handle, lab, np.array([255, 0, 1, 51], dtype='uint8').reshape(1, 1, 4))
    assert got[0, 2] == 1.0 and got[2, 2] == float(np.float32(1) / np.float32(255))


def test_ids(gpu_handle):
    """The sort's high bits; 2^53 has no exact place in a float64 row."""
    ids = np.array([0, 1, 2 ** 32 + 1, 2 ** 40, 2 ** 53 - 1], dtype=np.uint64)
    rng = np.random.RandomState(2)
    lab = ids[rng.randint(0, len(ids), (3, 6, 70))]
    data = _summable(rng, lab.shape, 'float32')
    got = _check(gpu_handle, lab, data, None)
    assert got[:, 0].tolist() == [float(i) for i in ids] and got[0, 1] > 0
    assert int(got[-1, 0]) == 2 ** 53 - 1
    lab[1, 1, 2] = 2 ** 53
    with pytest.raises(ctws.CtwsError, match='2\\^53'):
        gpu_handle.region_features_block(lab, data)
    ret, m, rows = gpu_handle.region_features_block_raw(lab, data, 0, 8)
    assert ret == -5 and m == 0 and np.isnan(rows).all()  # CTWS_EUNSUPPORTED, nothing written


@pytest.mark.parametrize('ignore_label', [0, 17, None, 999])
def test_ignore_label(gpu_handle, ignore_label):
    lab = _coherent(3, (5, 9, 70), (2, 4, 16), n_ids=30)
    assert (lab == 0).any() and (lab == 17).any() and not (lab == 999).any()
    data = _summable(np.random.RandomState(4), lab.shape, 'uint8')
    got = _check(gpu_handle, lab, data, ignore_label)
    zero = got[:, 1] == 0
    assert got[zero, 0].tolist() == ([float(ignore_label)] if ignore_label in (0, 17) else [])
    assert not got[zero, 2].any()
    assert got[:, 1].sum() == lab.size - (int((lab == ignore_label).sum()) if ignore_label is not None else 0)


def test_all_ignore_block_gives_one_row(gpu_handle):
    data = np.full((2, 3, 70), .25, dtype='float32')
    assert _check(gpu_handle, np.zeros((2, 3, 70)), data).tolist() == [[0, 0, 0]]
    assert _check(gpu_handle, np.full((2, 3, 70), 6), data, 6).tolist() == [[6, 0, 0]]
    assert _check(gpu_handle, np.zeros((2, 3, 70)), data, None).tolist() == [[0, 420, .25]]


K = 2048  # kRegfeatChunk: sorted records per chunk of k_regfeat_chunks / k_regfeat_rows


def _segment(lab, i):
    """[first, end) of id i among the sorted records of lab, from a CPU sort of the run heads (a
    head: a word's first voxel, or a voxel whose predecessor in the row holds another id)."""
    rows = lab.reshape(-1, lab.shape[2])
    head = np.ones(rows.shape, dtype=bool)
    head[:, 1:] = rows[:, 1:] != rows[:, :-1]
    head[:, ::64] = True
    keys = np.sort(rows[head], kind='stable')
    return int(np.searchsorted(keys, i, 'left')), int(np.searchsorted(keys, i, 'right'))


@pytest.mark.parametrize('front,back', [(0, 0), (1, 0), (700, 300), (2047, 1), (2048, 2047)])
def test_long_segments_are_split(gpu_handle, front, back):
    """An id whose segment of the sorted records holds whole aligned chunks of 2,048: those go to
    waves of their own and meet the segment's head [first, first chunk border) and tail in the
    id's wave through the chunk table.  Id 0 owns the records [0, 8192); `front` records of an id
    between the two come before the long segment of 2^40 + 7 and nothing compensates, so that
    segment starts at 8192 + front: on a chunk border (0, 2048), one past (1), between (700) and one
    before (2047).  `back` records of a larger id end it the same way."""
    big = 2 ** 40 + 7
    lab = np.empty((4, 16, 256), dtype=np.uint64)
    lab[:, :, 0::2] = 0  # alternating voxels: 8192 runs of length 1 each
    lab[:, :, 1::2] = big
    flat = lab.reshape(-1)
    flat[1:2 * front:2] = 2 ** 39               # the first `front` records of `big` go to a smaller id
    flat[flat.size - 2 * back + 1::2] = 2 ** 41  # and its last `back` records to a larger one
    first, end = _segment(lab, big)
    assert (first, end) == (8192 + front, 16384 - back) and _segment(lab, 0) == (0, 8192)
    assert first % K == front % K and end % K == -back % K
    assert end // K - -(-first // K) >= 1  # at least one whole aligned chunk inside
    rng = np.random.RandomState(front)
    for dtype in ('float32', 'uint8'):
        data = _summable(rng, lab.shape, dtype)
        got = _check(gpu_handle, lab, data, None)
        assert got[:, 0].tolist() == [0.] + ([2. ** 39] if front else []) + [float(big)] + ([2. ** 41] if back else [])
        assert got[0, 1] == 8192 and got[got[:, 0] == big, 1] == 8192 - front - back
        assert gpu_handle.region_features_block(lab, data, None).tobytes() == got.tobytes()


def test_one_long_segment_beside_many_short_ones(gpu_handle):
    """A background id owning most of the voxels among fragments of a few records each; its id is
    the largest, so its segment starts behind all of theirs, off a chunk border."""
    rng = np.random.RandomState(8)
    back = 1000
    lab = np.full((6, 30, 130), back, dtype=np.uint64)
    dots = rng.rand(*lab.shape) < .3
    lab[dots] = rng.randint(1, 400, int(dots.sum()))
    first, end = _segment(lab, back)
    assert first % K not in (0, 1) and end % K and end // K - -(-first // K) >= 1  # head, chunk(s), tail
    data = _summable(rng, lab.shape, 'float32')
    got = _check(gpu_handle, lab, data, None)
    assert got[-1, 0] == back and got[-1, 1] > .6 * lab.size and len(got) == 400
    assert dict(gpu_handle.timings())['regfeat_records'] == end
    got = _check(gpu_handle, lab, data, back)
    assert got[-1].tolist() == [back, 0, 0]


def test_general_floats(gpu_handle):
    """float32 values of both signs over 20 orders of magnitude: for every id |mean - S / n| <=
    (n + 2) 2^-53 sum|x| / n, S the exact sum -- gamma_(n-1) for a float64 sum of n terms in any
    order, the rounding of S itself and the division.  Repeated calls, the host-pointer call and the
    device-tensor call give identical bytes."""
    import torch
    rng = np.random.RandomState(9)
    lab = _coherent(7, (6, 20, 130), (3, 7, 23))
    data = (np.exp(rng.randn(*lab.shape) * 8) * rng.choice([-1., 1.], lab.shape)).astype('float32')
    assert np.isfinite(data).all()
    got = gpu_handle.region_features_block(lab, data)
    t = dict(gpu_handle.timings())
    for name in ('regfeat_count', 'regfeat_runs', 'regfeat_sort', 'regfeat_rows', 'regfeat_records'):
        assert name in t, (name, sorted(t))
    assert lab.size / 64 <= t['regfeat_records'] <= lab.size
    ids = np.unique(lab)
    assert got[:, 0].tolist() == [float(i) for i in ids]
    worst = 0.
    for i, n, mean in got:
        x = data[lab == i].astype('float64').tolist()
        if i == 0:
            assert n == 0 and mean == 0
            continue
        assert n == len(x)
        exact = sum((Fraction(v) for v in x), Fraction(0)) / len(x)
        bound = Fraction(len(x) + 2) * Fraction(R.U) * sum((Fraction(abs(v)) for v in x), Fraction(0)) / len(x)
        err = abs(Fraction(float(mean)) - exact)
        worst = max(worst, float(err / bound))
        assert err <= bound, (int(i), len(x), float(err), float(bound))
    print('largest error over bound: %.3g' % worst)
    for _ in range(5):
        assert gpu_handle.region_features_block(lab, data).tobytes() == got.tobytes()
    d = gpu_handle.region_features_block_device(torch.from_numpy(lab.view(np.int64)).cuda(),
                                                torch.from_numpy(data).cuda())
    assert d.is_cuda and d.dtype == torch.float64
    assert d.cpu().numpy().tobytes() == got.tobytes()


def test_device_path_dtypes(gpu_handle):
    import torch
    rng = np.random.RandomState(12)
    lab = _coherent(11, (3, 8, 70), (1, 2, 7), n_ids=30)
    tl = torch.from_numpy(lab.view(np.int64)).cuda()
    for dtype in ('uint8', 'float64'):
        data = _summable(rng, lab.shape, dtype)
        d = gpu_handle.region_features_block_device(tl, torch.from_numpy(data).cuda(), None)
        np.testing.assert_array_equal(d.cpu().numpy(), R.block_rows(lab, data, None))


def test_capacity(gpu_handle):
    lab = _coherent(5, (4, 10, 70), (2, 3, 11), n_ids=20)
    data = _summable(np.random.RandomState(5), lab.shape, 'uint16')
    want = R.block_rows(lab, data, 0)
    m = len(want)
    assert m > 10
    ret, got_m, rows = gpu_handle.region_features_block_raw(lab, data, 0, m - 1)
    assert ret == -1 and got_m == m and np.isnan(rows).all()  # CTWS_EINVAL, n_rows set, nothing written
    assert 'capacity' in lib().ctws_last_error(gpu_handle._h).decode()
    ret, got_m, rows = gpu_handle.region_features_block_raw(lab, data, 0, m)
    assert ret == 0 and got_m == m
    np.testing.assert_array_equal(rows, want)
    # a zero capacity without a buffer
    n = C.c_int64(-1)
    ret = lib().ctws_region_features_block(gpu_handle._h, lab.ctypes.data, data.ctypes.data, 2, *lab.shape, 1, 0,
                                           None, 0, C.byref(n))
    assert ret == -1 and n.value == m
    # a dtype code that is none of the four
    ret = lib().ctws_region_features_block(gpu_handle._h, lab.ctypes.data, data.ctypes.data, 9, *lab.shape, 1, 0,
                                           rows.ctypes.data, m, C.byref(n))
    assert ret == -1 and n.value == 0


def test_retry_on_capacity(gpu_handle, monkeypatch):
    import torch
    lab = _coherent(6, (3, 8, 70), (1, 2, 7), n_ids=30)
    data = _summable(np.random.RandomState(6), lab.shape, 'float32')
    monkeypatch.setattr(ctws.Handle, 'REGION_FEATURES_CAP', 4)
    _check(gpu_handle, lab, data)
    d = gpu_handle.region_features_block_device(torch.from_numpy(lab.view(np.int64)).cuda(),
                                                torch.from_numpy(data).cuda())
    np.testing.assert_array_equal(d.cpu().numpy(), R.block_rows(lab, data, 0))


def test_python_refusals(gpu_handle):
    lab = np.ones((2, 2, 3), dtype=np.uint64)
    data = np.ones((2, 2, 3), dtype='float32')
    f = gpu_handle.region_features_block
    with pytest.raises(TypeError, match='uint64'):
        f(lab.astype(np.int64), data)
    with pytest.raises(TypeError, match='uint8, uint16, float32 or float64'):
        f(lab, data.astype('int32'))
    with pytest.raises(TypeError):
        f(lab, data.astype('float16'))
    with pytest.raises(ValueError, match='one shape'):
        f(lab, data[:, :, :2])
    with pytest.raises(ValueError, match='3-D'):
        f(lab[0], data[0])
    with pytest.raises(ValueError, match='non-empty'):
        f(lab[:0], data[:0])
    f(lab, data)
    # the raw entry point refuses the same inputs
    raw = gpu_handle.region_features_block_raw
    with pytest.raises(TypeError, match='uint64'):
        raw(lab.astype(np.int64), data, 0, 4)
    with pytest.raises(TypeError, match='uint8, uint16, float32 or float64'):
        raw(lab, data.astype('int32'), 0, 4)
    with pytest.raises(ValueError, match='one shape'):
        raw(lab, data[:, :, :2], 0, 4)
    with pytest.raises(ValueError, match='3-D'):
        raw(lab[0], data[0], 0, 4)


def test_row_limit(gpu_handle):
    """2^31 - 1 rows of one voxel pass the voxel limit, but the scan of the rows' counts (and the 0
    behind them) is 32-bit: refused before any memory is touched."""
    lab = np.ones((1, 1, 4), dtype=np.uint64)
    data = np.ones((1, 1, 4), dtype='float32')
    rows = np.full((4, 3), np.nan)
    n = C.c_int64(-1)
    for shape in ((2 ** 31 - 1, 1, 1), (1, 2 ** 31 - 1, 1), (2 ** 16, 2 ** 15, 1), (2 ** 11, 2 ** 10, 2 ** 10)):
        ret = lib().ctws_region_features_block(gpu_handle._h, lab.ctypes.data, data.ctypes.data, 3, *shape, 1, 0,
                                               rows.ctypes.data, 4, C.byref(n))
        assert ret == -5 and n.value == 0 and np.isnan(rows).all(), shape
        assert '2^31' in lib().ctws_last_error(gpu_handle._h).decode()
