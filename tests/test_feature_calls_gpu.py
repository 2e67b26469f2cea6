"""One Handle through every feature block call in turn, on a block, a larger one and the first
again, then once more in the reverse order.  The calls share their staging and record buffers, the
counter block and the host code that drives them, so what this looks for is what no feature's own
file can see: a buffer left at the capacity of the call before, or a counter word that the feature
before wrote and this one reads.  Every result is compared with the restatement of its own test
file, and the first and third results of a feature must be the same bytes.

The larger block is arange + 1: every voxel an id of its own, so every counted emit (pairs and node
ids, overlap runs, morphology runs, edge samples) overflows its first buffer and runs twice."""
import numpy as np
import pytest

from cluster_tools_amd import ctws
import graph_ref as G
import node_labels_ref as NL
import morphology_ref as MO
import region_features_ref as RF
import edge_features_ref as EF
import downscaling_ref as DS

pytestmark = pytest.mark.gpu

BEGIN = (8, 16, 64)
FACTORS = (2, 2, 2)
FEATURES = ('rag', 'overlaps', 'morphology', 'region', 'edge', 'pairs', 'downscale')
# the pass count each counted emit reports, by feature
PASSES = {'rag': 'rag_pair_passes', 'overlaps': 'ov_pair_passes', 'morphology': 'morph_run_passes',
          'edge': 'ef_sample_passes'}


def _coherent(seed, shape, cell, n_ids=40):
    """Fragments: a coarse random grid enlarged to cells, with sprinkled single voxels (as
    test_morphology_gpu.py builds them)."""
    rng = np.random.RandomState(seed)
    coarse = rng.randint(0, n_ids, tuple(-(-s // c) for s, c in zip(shape, cell))).astype(np.uint64)
    vol = np.kron(coarse, np.ones(cell, dtype=np.uint64))[tuple(slice(0, s) for s in shape)]
    vol = np.ascontiguousarray(vol)
    vol[rng.rand(*shape) < .01] = n_ids + 1
    return vol


def _block(labels, seed):
    """The inputs of one block and the restatement of every feature on it."""
    rng = np.random.RandomState(seed)
    labels = np.ascontiguousarray(labels, dtype=np.uint64)
    labels2 = _coherent(seed + 1, labels.shape, (2, 3, 9), n_ids=7)
    # multiples of 2^-10 in [0, 1): float32 values whose sums are exact in any order
    data = (rng.randint(0, 1024, labels.shape) / 1024.).astype('float32')
    flat = labels.ravel()
    pairs = np.stack([flat[:-1], flat[1:]], axis=1)
    graph = G.rag(labels, True)
    uniq, counts = np.unique(pairs, axis=0, return_counts=True)
    want = {'rag': graph,
            'overlaps': (NL.overlap_rows(labels, labels2, None),),
            'morphology': (MO.block_morphology(labels, BEGIN),),
            'region': (RF.block_rows(labels, data, 0),),
            'edge': EF.block_features(labels, data, graph[1], True),
            'pairs': (uniq, counts.astype(np.uint64)),
            'downscale': (DS.reduce_block(data, FACTORS, 'mean'), True)}
    return dict(labels=labels, labels2=labels2, data=data, pairs=pairs, want=want)


@pytest.fixture(scope='module')
def blocks():
    small = _block(_coherent(3, (3, 5, 70), (2, 2, 16)), 1)
    large = _block(np.arange(5 * 6 * 67).reshape(5, 6, 67) + 1, 2)
    assert len(large['want']['rag'][1]) == 5263  # every face pair an edge of its own
    return small, large


def _call(h, name, b, graph):
    lab, data = b['labels'], b['data']
    if name == 'rag':
        return h.rag_block(lab, True)
    if name == 'overlaps':
        return (h.label_overlaps(lab, b['labels2'], None),)
    if name == 'morphology':
        return (h.block_morphology(lab, BEGIN),)
    if name == 'region':
        return (h.region_features_block(lab, data, 0),)
    if name == 'edge':
        return h.edge_features_block(lab, data, graph[0], graph[1], True)
    if name == 'pairs':
        return h.unique_pairs_u64(b['pairs'])
    return h.downscale_block(data, FACTORS, 'mean')


def _compare(name, got, want):
    assert len(got) == len(want)
    if name == 'edge':
        EF.compare(got[0], want[0])
        assert got[1] == want[1] == 0
        return
    for g, w in zip(got, want):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
            np.testing.assert_array_equal(g, w, err_msg=name)
        else:
            assert g is w, (name, g, w)


def test_one_handle_every_feature_growing_and_shrinking(blocks):
    small, large = blocks
    with ctws.Handle(0) as h:
        graphs = {}  # the graph rag_block gave for a block: the edge features' tables
        for order in (FEATURES, FEATURES[::-1]):
            results = {name: [] for name in FEATURES}
            for b in (small, large, small):
                for name in order:
                    # (in the reverse order the edge features come first: the graph of the round before)
                    got = _call(h, name, b, graphs.get(id(b)))
                    if name in PASSES and b is large:
                        assert h.timings()[PASSES[name]] == 2., name
                    _compare(name, got, b['want'][name])
                    if name == 'rag':
                        graphs[id(b)] = got
                    results[name].append(got)
            for name, (first, _, third) in results.items():
                for a, c in zip(first, third):
                    same = a.tobytes() == c.tobytes() if isinstance(a, np.ndarray) else a == c
                    assert same, (name, 'first and third call differ')
