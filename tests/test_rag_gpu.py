"""ctws_rag_block / ctws_unique_pairs_u64 on the GPU against the CPU restatement
(tests/graph_ref.py): nodes, edges and the voxel-pair counts per edge are all array_equal.  The
counts are what catch a lost or doubled emission that another voxel pair of the same edge would
hide; their sum must be the number of differing, not ignored face pairs."""
import numpy as np
import pytest

import graph_ref as G

pytestmark = pytest.mark.gpu


def _check(h, seg, ignore_label, ref=None):
    seg = np.ascontiguousarray(seg, dtype=np.uint64)
    ref = G.rag(seg, ignore_label) if ref is None else ref
    res = h.rag_block(seg, ignore_label)
    for got, want in zip(res, ref):
        assert got.dtype == np.uint64 and got.shape == want.shape, (got.shape, want.shape)
        np.testing.assert_array_equal(got, want)
    assert int(res[2].sum()) == G.n_face_pairs(seg, ignore_label)
    return res


@pytest.fixture(scope='module')
def documented():
    """The documented block with its restatements; the figures were computed on the CPU."""
    seg = G.documented_case()
    refs = {ign: G.rag(seg, ign) for ign in (False, True)}
    assert [len(t) for t in refs[False]] == [25, 82, 82] and int(refs[False][2].sum()) == 4152
    assert [len(t) for t in refs[True]] == [24, 80, 80] and int(refs[True][2].sum()) == 3972
    return seg, refs


@pytest.mark.parametrize('ignore_label', [False, True])
def test_documented_block(gpu_handle, documented, ignore_label):
    seg, refs = documented
    _check(gpu_handle, seg, ignore_label, refs[ignore_label])


@pytest.mark.parametrize('ignore_label', [False, True])
def test_every_pair_its_own_edge(gpu_handle, ignore_label):
    """The worst case for the pair buffer (3 emits per voxel against a first buffer of a quarter
    of the voxels): the emission is repeated at the counted size and loses nothing."""
    seg = (np.arange(5 * 6 * 67).reshape(5, 6, 67) + 1).astype(np.uint64)
    nodes, edges, counts = _check(gpu_handle, seg, ignore_label)
    assert len(nodes) == seg.size and len(edges) == 5263 and (counts == 1).all()
    assert gpu_handle.timings()['rag_pair_passes'] == 2.


def _far_face_cases():
    a = np.ones((3, 4, 130), np.uint64)
    a[:, :, 64:] = 2  # split between lanes 63 | 64 of the first word
    yield 'x64of130', a, 12
    for shape in ((3, 4, 130), (3, 4, 64), (1, 1, 65)):
        nz, ny, nx = shape
        if nx > 1:
            a = np.ones(shape, np.uint64)
            a[:, :, nx - 1] = 2
            yield 'x_last_%s' % (shape,), a, nz * ny
        if ny > 1:
            a = np.ones(shape, np.uint64)
            a[:, ny - 1, :] = 2
            yield 'y_last_%s' % (shape,), a, nz * nx
        if nz > 1:
            a = np.ones(shape, np.uint64)
            a[nz - 1] = 2
            yield 'z_last_%s' % (shape,), a, ny * nx


@pytest.mark.parametrize('name,seg,n_pairs', list(_far_face_cases()), ids=[c[0] for c in _far_face_cases()])
def test_boundary_only_at_far_face(gpu_handle, name, seg, n_pairs):
    for ignore_label in (False, True):
        nodes, edges, counts = _check(gpu_handle, seg, ignore_label)
        assert nodes.tolist() == [1, 2] and edges.tolist() == [[1, 2]] and counts.tolist() == [n_pairs]


def test_degenerate_blocks(gpu_handle):
    const = np.full((3, 5, 70), 7, np.uint64)
    for ignore_label in (False, True):
        nodes, edges, counts = _check(gpu_handle, const, ignore_label)
        assert nodes.tolist() == [7] and edges.shape == (0, 2) and counts.shape == (0,)
        assert gpu_handle.timings()['rag_pair_passes'] == 1.  # no pair and one node id: both fit
    zero = np.zeros((3, 5, 70), np.uint64)
    nodes, edges, counts = _check(gpu_handle, zero, True)
    assert nodes.shape == (0,) and edges.shape == (0, 2) and counts.shape == (0,)
    nodes, edges, counts = _check(gpu_handle, zero, False)
    assert nodes.tolist() == [0] and edges.shape == (0, 2)
    one = np.full((1, 1, 1), 5, np.uint64)
    assert _check(gpu_handle, one, True)[0].tolist() == [5]


@pytest.mark.parametrize('ignore_label', [False, True])
def test_large_ids(gpu_handle, documented, ignore_label):
    seg, refs = documented
    big = np.where(seg != 0, seg + np.uint64(2 ** 33), np.uint64(0))
    nodes, edges, counts = _check(gpu_handle, big, ignore_label)
    # the same graph, shifted
    shift = lambda t: np.where(t != 0, t + np.uint64(2 ** 33), np.uint64(0))
    np.testing.assert_array_equal(nodes, shift(refs[ignore_label][0]))
    np.testing.assert_array_equal(edges, shift(refs[ignore_label][1]))
    np.testing.assert_array_equal(counts, refs[ignore_label][2])


@pytest.mark.parametrize('ignore_label', [False, True])
def test_extreme_ids_in_slabs(gpu_handle, ignore_label):
    ids = np.array([1, 2 ** 32, 2 ** 63, 2 ** 64 - 1, 0], dtype=np.uint64)
    seg = np.zeros((4, 10, 70), np.uint64)
    for k in range(5):
        seg[:, 2 * k:2 * k + 2, :] = ids[k]
    seg[2:, :, 40:] = seg[2:, ::-1, 40:]  # every id meets others across x and z too
    nodes, edges, counts = _check(gpu_handle, seg, ignore_label)
    assert nodes.tolist() == sorted(ids.tolist())[1 if ignore_label else 0:]
    assert [2 ** 63, 2 ** 64 - 1] in edges.tolist()


def test_device_path_equals_host_path(gpu_handle, documented):
    import torch
    seg, refs = documented
    for ignore_label in (False, True):
        t = torch.from_numpy(seg.view(np.int64)).to('cuda:0')
        res = gpu_handle.rag_block_device(t, ignore_label)
        assert all(r.is_cuda and r.dtype == torch.int64 for r in res)
        host = gpu_handle.rag_block(seg, ignore_label)
        for got, want, ref in zip(res, host, refs[ignore_label]):
            got = got.cpu().numpy().view(np.uint64)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(got, ref)
        np.testing.assert_array_equal(t.cpu().numpy().view(np.uint64), seg)  # the labels are only read


def test_small_caps(gpu_handle, documented):
    seg, refs = documented
    nodes_ref, edges_ref, counts_ref = refs[True]
    for cn, ce in ((0, 0), (3, 1000), (1000, 5), (len(nodes_ref) - 1, len(edges_ref)),
                   (len(nodes_ref), len(edges_ref) - 1)):
        ret, nn, ne, _, _, _ = gpu_handle.rag_block_raw(seg, True, cn, ce)
        assert ret == -1 and (nn, ne) == (len(nodes_ref), len(edges_ref)), (cn, ce, ret, nn, ne)
        assert 'capacity' in gpu_handle.last_error()
    ret, nn, ne, nodes, edges, counts = gpu_handle.rag_block_raw(seg, True, len(nodes_ref), len(edges_ref))
    assert ret == 0 and (nn, ne) == (len(nodes_ref), len(edges_ref))
    np.testing.assert_array_equal(nodes, nodes_ref)
    np.testing.assert_array_equal(edges, edges_ref)
    np.testing.assert_array_equal(counts, counts_ref)


def test_call_repeated_with_returned_sizes(gpu_handle, documented, monkeypatch):
    """Handle.rag_block[_device] repeat a call that hits a capacity once, with the sizes it returned."""
    import torch
    seg, refs = documented
    monkeypatch.setattr(gpu_handle, 'RAG_CAPS', (2, 3), raising=False)
    _check(gpu_handle, seg, True, refs[True])
    res = gpu_handle.rag_block_device(torch.from_numpy(seg.view(np.int64)).to('cuda:0'), True)
    for got, want in zip(res, refs[True]):
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), want)


def test_deterministic(gpu_handle, documented):
    seg, _ = documented
    first = gpu_handle.rag_block(seg, True)
    for _ in range(2):
        for got, want in zip(gpu_handle.rag_block(seg, True), first):
            np.testing.assert_array_equal(got, want)


def _np_unique_pairs(pairs, weights=None):
    uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
    w = np.ones(len(pairs), np.uint64) if weights is None else weights
    sums = np.zeros(len(uniq), np.uint64)
    np.add.at(sums, inv.ravel(), w)
    return uniq, sums


@pytest.mark.parametrize('weighted', [False, True])
def test_unique_pairs_random(gpu_handle, weighted):
    rng = np.random.RandomState(5)
    ids = np.unique(rng.randint(0, 2 ** 62, 300).astype(np.uint64) * np.uint64(3))
    ids[:3] = [0, 2 ** 64 - 1, 2 ** 32]
    pairs = ids[rng.randint(0, len(ids), (100000, 2))]
    weights = rng.randint(0, 1000, len(pairs)).astype(np.uint64) if weighted else None
    uniq, sums = _np_unique_pairs(pairs, weights)
    assert len(uniq) < len(pairs)  # duplicates
    got, got_sums = gpu_handle.unique_pairs_u64(pairs, weights)
    assert got.dtype == got_sums.dtype == np.uint64
    np.testing.assert_array_equal(got, uniq)
    np.testing.assert_array_equal(got_sums, sums)


def test_unique_pairs_edge_cases(gpu_handle):
    got, sums = gpu_handle.unique_pairs_u64(np.zeros((0, 2), np.uint64))
    assert got.shape == (0, 2) and sums.shape == (0,)
    big = 2 ** 64 - 1
    pairs = np.array([[big, big], [0, big], [big, 0], [0, big], [big, big], [5, 5]], dtype=np.uint64)
    got, sums = gpu_handle.unique_pairs_u64(pairs)
    assert got.tolist() == [[0, big], [5, 5], [big, 0], [big, big]] and sums.tolist() == [2, 1, 1, 2]
    # the capacity contract of ctws_unique_u64: the size is returned with CTWS_EINVAL
    ret, m, _, _ = gpu_handle.unique_pairs_u64_raw(pairs, None, 3)
    assert ret == -1 and m == 4
    ret, m, out, cnt = gpu_handle.unique_pairs_u64_raw(pairs, None, 4)
    assert ret == 0 and m == 4 and out.tolist() == got.tolist() and cnt.tolist() == sums.tolist()
