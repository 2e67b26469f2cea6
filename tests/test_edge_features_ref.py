"""The CPU restatement of the edge features (tests/edge_features_ref.py) against a triple-loop brute
force, and its block / merge / whole-volume consistency on the workflow tests' volume: every voxel
pair is owned by exactly one block, so the merged count, min, max, mean and variance equal the
whole-volume features (the merged quantiles are weighted averages and do not)."""
import numpy as np
import pytest

from cluster_tools_amd.utils.blocking import Blocking
from cluster_tools_amd.graph.map_edge_ids import EdgeIndex
import graph_ref as G
import edge_features_ref as E

SHAPE = (20, 48, 80)
BLOCK_SHAPE = [8, 32, 32]


def _tiny(seed, shape=(5, 6, 7), n_ids=5):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n_ids, shape).astype(np.uint64), rng.random(shape, dtype=np.float32)


@pytest.mark.parametrize('ignore_label', [True, False])
@pytest.mark.parametrize('core', [None, (4, 5, 6), (5, 5, 7), (2, 6, 3)])
def test_restatement_equals_brute_force(ignore_label, core):
    for seed in range(3):
        labels, data = _tiny(seed)
        edges = G.rag(labels, ignore_label)[1]
        got, miss = E.block_features(labels, data, edges, ignore_label, core)
        ref, miss_ref = E.block_features_brute(labels, data, edges, ignore_label, core)
        assert miss == miss_ref == 0
        np.testing.assert_array_equal(got, ref)
        assert got[:, 9].sum() > 0


def test_restatement_details():
    labels, data = _tiny(7)
    data = (data * 2 - 1).astype(np.float32)
    data[0, 0, 0] = -0.0
    edges, counts = G.rag(labels, True)[1:]
    got, _ = E.block_features(labels, data, edges, True)
    np.testing.assert_array_equal(got, E.block_features_brute(labels, data, edges, True)[0])
    np.testing.assert_array_equal(got[:, 9], counts)
    assert (got[:, 2] < 0).any() and np.all(got[:, 2] <= got[:, 5]) and np.all(got[:, 5] <= got[:, 8])
    # uint8 input is v / 255 in float32
    u8 = np.random.default_rng(1).integers(0, 256, labels.shape).astype(np.uint8)
    a, _ = E.block_features(labels, u8, edges, True)
    b, _ = E.block_features(labels, u8.astype(np.float32) / np.float32(255), edges, True)
    np.testing.assert_array_equal(a, b)
    assert a[:, 8].max() <= 1.
    # an edge missing from the table: its pairs are counted, the other rows stay
    less, miss = E.block_features(labels, data, np.delete(edges, 2, axis=0), True)
    assert miss == counts[2] > 0
    np.testing.assert_array_equal(less, np.delete(got, 2, axis=0))
    assert E.block_features_brute(labels, data, np.delete(edges, 2, axis=0), True)[1] == miss
    # two samples: every quantile interpolates between them
    row = E.row_of([0.25, 0.75], 1)
    np.testing.assert_allclose(row, [0.5, 0.0625, 0.25, 0.3, 0.375, 0.5, 0.625, 0.7, 0.75, 1.], rtol=0, atol=1e-15)


class _Volume:
    def __init__(self):
        self.seg = G.workflow_volume()
        self.data = np.random.default_rng(0).random(SHAPE, dtype=np.float32)
        self.blocking = Blocking([0, 0, 0], list(SHAPE), BLOCK_SHAPE)
        assert self.blocking.numberOfBlocks == 18


@pytest.fixture(scope='module')
def volume():
    return _Volume()


@pytest.mark.parametrize('ignore_label,n_global', [(False, 181), (True, 167)])
def test_blocks_merge_to_the_whole_volume(volume, ignore_label, n_global):
    seg, data = volume.seg, volume.data
    _, edges, counts = G.rag(seg, ignore_label)
    assert len(edges) == n_global
    whole, miss = E.block_features(seg, data, edges, ignore_label)
    assert miss == 0
    np.testing.assert_array_equal(whole[:, 9], counts)
    index = EdgeIndex(edges)
    blocks, n_zero_rows, n_edgeless = [], 0, 0
    for block_id in range(18):
        bb = G.extended_box(volume.blocking, block_id, SHAPE)
        sub = G.rag(seg[bb], ignore_label)[1]
        feats, miss = E.block_features(seg[bb], data[bb], sub, ignore_label, E.core_shape(volume.blocking, block_id))
        assert miss == 0 and feats.shape == (len(sub), 10)
        n_zero_rows += int((feats[:, 9] == 0).sum())
        n_edgeless += len(sub) == 0
        assert not feats[feats[:, 9] == 0].any()
        blocks.append((index.edge_ids(sub), feats))
    # the case is not hollow: halo-plane-only edges and edge-less blocks exist
    assert n_zero_rows == 21 and n_edgeless == 2
    merged = E.merge_features(len(edges), blocks)
    for col in (9, 2, 8):
        np.testing.assert_array_equal(merged[:, col], whole[:, col])
    np.testing.assert_allclose(merged[:, 0], whole[:, 0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(merged[:, 1], whole[:, 1], rtol=0, atol=1e-12)
    # the merged quantiles are weighted averages: approximate by nature, compared with nothing else
    assert np.abs(merged[:, 5] - whole[:, 5]).max() > 0.05


def test_merge_edge_without_rows_stays_zero():
    feats = np.array([[.5, .1, .2, .3, .4, .5, .6, .7, .8, 2.], [0.] * 10])
    merged = E.merge_features(4, [(np.array([1, 3]), feats), (np.array([1]), feats[:1] + 0.)])
    assert not merged[[0, 2, 3]].any()
    np.testing.assert_allclose(merged[1], [.5, .1, .2, .3, .4, .5, .6, .7, .8, 4.], rtol=0, atol=1e-15)
