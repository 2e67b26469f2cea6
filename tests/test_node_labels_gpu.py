"""ctws_label_overlaps on the GPU against the CPU restatement (tests/node_labels_ref.py): the
rows (node, label, count), their order and their counts are all array_equal.  The shapes are the
smallest that reach each path of the kernel: a tail wave, one run per wave, every lane a run
head (stage flushes and the second pass at the counted size), runs over the 64-lane boundary and
the row end, and ids at both ends of the uint64 range."""
import ctypes as C

import numpy as np
import pytest

import node_labels_ref as R

pytestmark = pytest.mark.gpu

U64_MAX = 2 ** 64 - 1


def _check(h, nodes, labels, ignore_label=None):
    want = R.overlap_rows(nodes, labels, ignore_label)
    got = h.label_overlaps(nodes, labels, ignore_label)
    assert got.dtype == np.uint64 and got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got, want)
    counted = np.asarray(labels).size if ignore_label is None else \
        int((np.asarray(labels).astype('uint64') != np.uint64(ignore_label & U64_MAX)).sum())
    assert int(got[:, 2].sum()) == counted
    return got


def _volumes(shape, seed, n_nodes=9, n_labels=5):
    """Coherent ids: runs of varying length along the flat index, so runs cross lanes 63 | 64 and row ends."""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    def runs(k):
        out = np.empty(n, np.uint64)
        pos = 0
        while pos < n:
            ln = int(rng.randint(1, 150))
            out[pos:pos + ln] = rng.randint(0, k)
            pos += ln
        return out.reshape(shape)
    return runs(n_nodes), runs(n_labels)


@pytest.mark.parametrize('ignore_label', [None, 0, 7])
def test_tail_wave(gpu_handle, ignore_label):
    """(3, 5, 67): a row length that is no multiple of 64 and a last word of 45 voxels."""
    nodes, labels = _volumes((3, 5, 67), 0, n_labels=9)
    nodes.reshape(-1)[50:80] = 0
    labels.reshape(-1)[60:70] = 7
    labels.reshape(-1)[300:420] = 0
    labels.reshape(-1)[990:] = 7  # into the tail word
    rows = _check(gpu_handle, nodes, labels, ignore_label)
    assert (rows[:, 0] == 0).any()  # node 0 is counted like any other


def test_single_voxel(gpu_handle):
    one = np.array([[[5]]], np.uint64)
    assert _check(gpu_handle, one, one + 1).tolist() == [[5, 6, 1]]
    assert _check(gpu_handle, one, one + 1, 6).shape == (0, 3)


def test_constant(gpu_handle):
    """(4, 8, 64): one run per wave, every emit the same pair."""
    nodes = np.full((4, 8, 64), 3, np.uint64)
    labels = np.full((4, 8, 64), 11, np.uint64)
    assert _check(gpu_handle, nodes, labels).tolist() == [[3, 11, 2048]]
    assert gpu_handle.timings()['ov_pair_passes'] == 1.  # 32 runs in a first buffer of 512


def test_every_voxel_distinct(gpu_handle):
    """(8, 16, 64) with random 64-bit node ids: every lane a run head, the stage is flushed every
    fourth word, the first buffer of a quarter of the voxels overflows and the sort has no duplicates."""
    rng = np.random.RandomState(1)
    nodes = rng.randint(0, 2 ** 63, size=(8, 16, 64)).astype(np.uint64) * np.uint64(2) + \
        rng.randint(0, 2, size=(8, 16, 64)).astype(np.uint64)
    assert len(np.unique(nodes)) == nodes.size
    labels = rng.randint(0, 3, size=nodes.shape).astype(np.uint64)
    rows = _check(gpu_handle, nodes, labels)
    assert len(rows) == nodes.size and (rows[:, 2] == 1).all()
    assert gpu_handle.timings()['ov_pair_passes'] == 2.


def test_one_pair_large(gpu_handle):
    nodes = np.full((16, 64, 128), 1, np.uint64)
    labels = np.full((16, 64, 128), 2, np.uint64)
    assert _check(gpu_handle, nodes, labels).tolist() == [[1, 2, 131072]]


def test_runs_cross_word_and_row(gpu_handle):
    """One run over lanes 60..70 of the flat index (it crosses the 64-lane boundary and, with
    rows of 67 voxels, the row end at 67) between two other pairs."""
    nodes = np.full((2, 3, 67), 1, np.uint64)
    labels = np.full((2, 3, 67), 1, np.uint64)
    nodes.reshape(-1)[60:71] = 2
    labels.reshape(-1)[65:200] = 4
    rows = _check(gpu_handle, nodes, labels)
    assert R.rows_to_dict(rows) == {1: {1: 60 + 202, 4: 129}, 2: {1: 5, 4: 6}}


@pytest.mark.parametrize('side', ['nodes', 'labels', 'both'])
def test_large_ids(gpu_handle, side):
    """ids above 2^32 and 2^64 - 1, on either side; 2^64 - 1 as the ignore label too."""
    nodes, labels = _volumes((3, 5, 67), 2)
    big = np.array([0, 1, 2 ** 32 + 5, 2 ** 40, 2 ** 63, U64_MAX - 1, U64_MAX, 7, 2 ** 32, 3], np.uint64)
    if side in ('nodes', 'both'):
        nodes = big[nodes.astype(np.int64)]
    if side in ('labels', 'both'):
        labels = big[labels.astype(np.int64)]
    _check(gpu_handle, nodes, labels)
    _check(gpu_handle, nodes, labels, 0)
    if side != 'nodes':
        labels.reshape(-1)[:100] = U64_MAX
        rows = _check(gpu_handle, nodes, labels, U64_MAX)
        assert not (rows[:, 1] == np.uint64(U64_MAX)).any()


def test_all_ignored(gpu_handle):
    nodes, _ = _volumes((3, 5, 67), 3)
    labels = np.full(nodes.shape, 7, np.uint64)
    assert _check(gpu_handle, nodes, labels, 7).shape == (0, 3)
    assert len(_check(gpu_handle, nodes, labels, 0)) == len(np.unique(nodes))


def test_int32_labels_with_negatives(gpu_handle):
    """Any integer dtype goes through .astype('uint64'), as the reference does: -1 is 2^64 - 1."""
    nodes, labels = _volumes((3, 5, 67), 4)
    labels = labels.astype(np.int32) - 2
    labels.reshape(-1)[5:40] = -1
    labels.reshape(-1)[500:510] = -2
    rows = _check(gpu_handle, nodes, labels)
    assert (rows[:, 1] == np.uint64(U64_MAX)).any()
    rows = _check(gpu_handle, nodes, labels, -1)
    assert not (rows[:, 1] == np.uint64(U64_MAX)).any()


def test_capacity_protocol(gpu_handle):
    """cap one too small: CTWS_EINVAL, n_rows set, nothing written; the exact cap fits."""
    nodes, labels = _volumes((3, 5, 67), 5)
    want = R.overlap_rows(nodes, labels)
    m = len(want)
    assert m > 1
    from cluster_tools_amd.ctws import lib
    rows = np.full((m, 3), 0xABCD, np.uint64)
    n = C.c_int64(-5)
    ret = lib().ctws_label_overlaps(gpu_handle._h, nodes.ctypes.data, labels.ctypes.data, nodes.size, 0, 0,
                                    rows.ctypes.data, m - 1, C.byref(n))
    assert ret == -1 and n.value == m and (rows == 0xABCD).all()
    ret, got_m, got = gpu_handle.label_overlaps_raw(nodes, labels, None, m)
    assert ret == 0 and got_m == m
    np.testing.assert_array_equal(got, want)


def test_device_and_repeat(gpu_handle):
    """Host and _device results identical; two repeated calls identical."""
    import torch
    nodes, labels = _volumes((5, 9, 130), 6)
    for ignore_label in (None, 0):
        a = gpu_handle.label_overlaps(nodes, labels, ignore_label)
        b = gpu_handle.label_overlaps(nodes, labels, ignore_label)
        assert a.tobytes() == b.tobytes()
        dn = torch.from_numpy(nodes.view(np.int64)).to('cuda:0')
        dl = torch.from_numpy(labels.view(np.int64)).to('cuda:0')
        d = gpu_handle.label_overlaps_device(dn, dl, ignore_label)
        assert d.is_cuda and d.dtype == torch.int64
        assert d.cpu().numpy().view(np.uint64).tobytes() == a.tobytes()
        np.testing.assert_array_equal(a, R.overlap_rows(nodes, labels, ignore_label))
