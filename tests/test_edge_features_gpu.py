"""ctws_edge_features_block on the GPU against the CPU restatement (tests/edge_features_ref.py):
count, min and max are array_equal, mean, variance and the quantiles agree within 1e-10 absolute.
The samples are float32-exact with magnitude at most 1 and the largest edge here has 16,640 of
them, so a float64 sum in any order is off by at most n 2^-53 ~ 2e-12; an order statistic picked
one place off differs by about a float32 spacing, 6e-8."""
import numpy as np
import pytest

import graph_ref as G
import edge_features_ref as E

pytestmark = pytest.mark.gpu

compare = E.compare


def _check(h, seg, data, ignore_label, core=None, graph=None):
    seg = np.ascontiguousarray(seg, dtype=np.uint64)
    nodes, edges, counts = G.rag(seg, ignore_label) if graph is None else graph
    ref, miss_ref = E.block_features(seg, data, edges, ignore_label, core)
    got, miss = h.edge_features_block(seg, data, nodes, edges, ignore_label, core)
    assert miss == miss_ref == 0
    compare(got, ref)
    return got, ref, counts


def _data(shape, seed=0):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


@pytest.fixture(scope='module')
def documented():
    """The documented block of the RAG tests with its restated graphs and a boundary map."""
    seg = G.documented_case()
    graphs = {ign: G.rag(seg, ign) for ign in (False, True)}
    assert [len(graphs[i][1]) for i in (False, True)] == [82, 80]
    assert [int(graphs[i][2].sum()) for i in (False, True)] == [4152, 3972]
    assert 2 * int(graphs[False][2].max()) == 654
    return seg, graphs, _data(seg.shape)


@pytest.mark.parametrize('ignore_label', [False, True])
def test_documented_block(gpu_handle, documented, ignore_label):
    seg, graphs, data = documented
    got, _, counts = _check(gpu_handle, seg, data, ignore_label, graph=graphs[ignore_label])
    # core == extended: the pair set is the RAG's
    np.testing.assert_array_equal(got[:, 9], gpu_handle.rag_block(seg, ignore_label)[2])
    np.testing.assert_array_equal(got[:, 9], counts)


@pytest.mark.parametrize('ignore_label', [False, True])
def test_core_box_owns_the_pairs(gpu_handle, documented, ignore_label):
    """Pairs wholly in the upper halo planes belong to the neighbouring block: fewer pairs, and an
    edge seen only there keeps its row with ten zeros."""
    seg, graphs, data = documented
    core = (8, 20, 69)
    got, ref, counts = _check(gpu_handle, seg, data, ignore_label, core, graphs[ignore_label])
    assert (ref[:, 9] == 0).any() and not ref[ref[:, 9] == 0].any()
    assert got[:, 9].sum() == ref[:, 9].sum() < counts.sum()
    # and a core that ends inside a word / before the last row and slice
    _check(gpu_handle, seg, data, ignore_label, (3, 7, 64), graphs[ignore_label])
    _check(gpu_handle, seg, data, ignore_label, (9, 21, 1), graphs[ignore_label])


def test_long_segment_beside_short_ones(gpu_handle):
    seg = np.ones((8, 64, 130), np.uint64)
    seg[4:] = 2
    seg[0, 0, 0] = 3
    got, ref, counts = _check(gpu_handle, seg, _data(seg.shape, 1), True)
    assert counts.tolist() == [64 * 130, 3] and 2 * int(counts[0]) == 16640
    assert gpu_handle.timings()['ef_sample_passes'] == 1.  # 16,646 keys in a first buffer of 33,280
    # one pair: every quantile lies between the only two samples
    seg[0, 0, 0] = 1
    seg[7, 63, 129] = 3
    got, ref, _ = _check(gpu_handle, seg, _data(seg.shape, 1), True, core=(8, 64, 129))
    assert ref[:, 9].tolist() == [64 * 129, 1]
    assert ref[1, 2] < ref[1, 3] < ref[1, 5] < ref[1, 7] < ref[1, 8]


@pytest.mark.parametrize('ignore_label', [False, True])
def test_uint8_data(gpu_handle, documented, ignore_label):
    seg, graphs, _ = documented
    data = np.random.default_rng(2).integers(0, 256, seg.shape).astype(np.uint8)
    got, _, _ = _check(gpu_handle, seg, data, ignore_label, graph=graphs[ignore_label])
    assert got[:, 2].min() == 0. and got[:, 8].max() == 1.


def test_constant_data(gpu_handle, documented):
    seg, graphs, _ = documented
    c = np.float32(0.3)
    got, _, _ = _check(gpu_handle, seg, np.full(seg.shape, c, np.float32), True, graph=graphs[True])
    assert (got[:, 1] == 0.).all()
    for col in (0, 2, 3, 4, 5, 6, 7, 8):
        np.testing.assert_array_equal(got[:, col], np.full(len(got), float(c)))


def test_negative_values_and_negative_zero(gpu_handle, documented):
    seg, graphs, data = documented
    data = (2 * data - 1).astype(np.float32)
    data[::2, ::3, ::5] = -0.0
    data[1::2, ::3, ::5] = 0.0
    data[0, 0, :4] = [-1., 1., -1., 1.]
    got, _, _ = _check(gpu_handle, seg, data, False, graph=graphs[False])
    assert got[:, 2].min() == -1. and got[:, 8].max() == 1. and (got[:, 5] < 0).any()


def test_large_ids(gpu_handle, documented):
    seg, graphs, data = documented
    big = np.where(seg != 0, seg + np.uint64(2 ** 33), np.uint64(0))
    got, _, _ = _check(gpu_handle, big, data, True)
    ref, _ = E.block_features(seg, data, graphs[True][1], True)
    compare(got, ref)
    ids = np.array([1, 2 ** 32, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)
    seg4 = ids[np.random.default_rng(4).integers(0, 4, (6, 9, 70))]
    got, _, counts = _check(gpu_handle, seg4, _data(seg4.shape, 4), False)
    assert len(got) == 6 and counts.min() > 0


@pytest.mark.parametrize('ignore_label', [False, True])
def test_every_pair_its_own_edge(gpu_handle, ignore_label):
    """5,263 edges of two samples, 10,526 keys against a first buffer of half the voxels: the
    sample pass is repeated at the counted size and loses nothing."""
    seg = (np.arange(5 * 6 * 67).reshape(5, 6, 67) + 1).astype(np.uint64)
    got, ref, _ = _check(gpu_handle, seg, _data(seg.shape, 5), ignore_label)
    assert len(got) == 5263 and (got[:, 9] == 1).all()
    assert gpu_handle.timings()['ef_sample_passes'] == 2.
    np.testing.assert_array_equal(got[:, 5], ref[:, 5])  # the mean of two float32 values is exact


def test_blocks_without_edges(gpu_handle):
    for seg, ign in ((np.full((4, 5, 70), 7, np.uint64), True), (np.zeros((4, 5, 70), np.uint64), True),
                     (np.zeros((4, 5, 70), np.uint64), False)):
        nodes, edges, _ = G.rag(seg, ign)
        assert len(edges) == 0
        got, miss = gpu_handle.edge_features_block(seg, _data(seg.shape), nodes, edges, ign)
        assert got.shape == (0, 10) and got.dtype == np.float64 and miss == 0


def test_missing_edge_is_counted(gpu_handle, documented):
    seg, graphs, data = documented
    nodes, edges, counts = graphs[True]
    full, _ = gpu_handle.edge_features_block(seg, data, nodes, edges, True)
    k = int(np.argmax(counts))
    got, miss = gpu_handle.edge_features_block(seg, data, nodes, np.delete(edges, k, axis=0), True)
    ref, miss_ref = E.block_features(seg, data, np.delete(edges, k, axis=0), True)
    assert miss == miss_ref == int(counts[k]) > 0
    np.testing.assert_array_equal(got, np.delete(full, k, axis=0))
    compare(got, ref)


def test_bad_inputs_fail_loudly(gpu_handle, documented):
    from cluster_tools_amd.ctws import CtwsError
    seg, graphs, data = documented
    nodes, edges, _ = graphs[True]
    with pytest.raises(TypeError):
        gpu_handle.edge_features_block(seg, data.astype(np.float64), nodes, edges, True)
    with pytest.raises(ValueError):
        gpu_handle.edge_features_block(seg[0], data[0], nodes, edges, True)
    with pytest.raises(ValueError):
        gpu_handle.edge_features_block(seg, data, nodes, edges, True, core_shape=(10, 21, 70))
    with pytest.raises(CtwsError, match='sorted'):
        gpu_handle.edge_features_block(seg, data, nodes, edges[::-1], True)
    with pytest.raises(CtwsError, match='missing from the nodes'):
        gpu_handle.edge_features_block(seg, data, nodes[1:], edges, True)


def test_device_tensors_and_reproducibility(gpu_handle, documented):
    import torch
    seg, graphs, data = documented
    nodes, edges, _ = graphs[True]
    core = (8, 20, 69)
    host = [gpu_handle.edge_features_block(seg, data, nodes, edges, True, core) for _ in range(3)]
    for got, miss in host[1:]:
        assert miss == 0
        np.testing.assert_array_equal(got, host[0][0])
    dev = torch.device('cuda', gpu_handle.device)
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(dev) for a in (seg, nodes, edges)]
    out, miss = gpu_handle.edge_features_block_device(t[0], torch.from_numpy(data).to(dev), t[1], t[2], True, core)
    assert miss == 0 and out.is_cuda and out.dtype == torch.float64
    np.testing.assert_array_equal(out.cpu().numpy(), host[0][0])
    u8 = np.random.default_rng(2).integers(0, 256, seg.shape).astype(np.uint8)
    out, _ = gpu_handle.edge_features_block_device(t[0], torch.from_numpy(u8).to(dev), t[1], t[2], True, core)
    np.testing.assert_array_equal(out.cpu().numpy(), gpu_handle.edge_features_block(seg, u8, nodes, edges, True, core)[0])
    empty = torch.zeros((0, 2), dtype=torch.int64, device=dev)
    out, miss = gpu_handle.edge_features_block_device(t[0], torch.from_numpy(data).to(dev), t[1], empty, True)
    assert tuple(out.shape) == (0, 10) and miss == 0
