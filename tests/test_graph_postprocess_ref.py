"""CPU checks of the restatement the GPU tests compare to (tests/graph_postprocess_ref.py) against
scipy's csgraph, an independent oracle: components against `connected_components` on the filtered
edge list, the flood on distinct weights against the labels read off `minimum_spanning_tree` of the
graph plus a virtual root, the flood against the Boruvka rounds where ties decide, and the host
helpers of the GraphWatershedAssignments job against the reference's lines."""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components, minimum_spanning_tree

from cluster_tools_amd.postprocess import graph_watershed_assignments as gws
import graph_postprocess_ref as R


def _by_smallest_node(labels, keep):
    """Component labels -> 1 + rank of the component's smallest node among the kept nodes' components."""
    out = np.zeros(len(labels), dtype='uint64')
    nodes = np.nonzero(keep)[0]
    smallest = np.full(int(labels.max()) + 1, len(labels), dtype='int64')
    np.minimum.at(smallest, labels[nodes], nodes)
    rank = np.argsort(np.argsort(smallest))  # components without a kept node sort last
    out[nodes] = rank[labels[nodes]] + 1
    return out


def _scipy_components(edges, assignments):
    n = len(assignments)
    e = edges.astype('int64')
    keep = (assignments[e[:, 0]] == assignments[e[:, 1]]) & (assignments[e[:, 0]] != 0)
    e = e[keep]
    g = coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n))
    return _by_smallest_node(connected_components(g, directed=False)[1], assignments != 0)


@pytest.mark.parametrize('seed', range(6))
def test_components_equal_scipy(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 300))
    edges = R.random_graph(rng, n, int(rng.integers(1, 3 * n)))
    for assignments in (rng.integers(0, 4, n), 1 + np.arange(n) % 3, np.ones(n), 1 + np.arange(n), np.zeros(n)):
        assignments = assignments.astype('uint64')
        assert np.array_equal(R.components(edges, assignments), _scipy_components(edges, assignments))
    assert np.array_equal(R.components(edges[::-1, ::-1], assignments), R.components(edges, assignments))


def test_components_small_cases():
    edges = np.array([[0, 1], [1, 2], [3, 4], [2, 5]], dtype='uint64')
    assert R.components(edges, np.array([7, 7, 7, 7, 7, 7])).tolist() == [1, 1, 1, 2, 2, 1]
    assert R.components(edges, np.array([7, 0, 7, 3, 3, 7])).tolist() == [1, 0, 2, 3, 3, 2]
    assert R.components(np.zeros((0, 2)), np.array([5, 0, 5])).tolist() == [1, 0, 2]
    with pytest.raises(ValueError):
        R.components(edges, np.ones(5))


def _mst_labels(edges, weights, seeds):
    """The watershed as the minimum spanning forest of the graph plus a virtual root that is
    joined to every seed by an edge lighter than all others: a node's label is the seed in its
    tree once the root is taken out.  Weights are positive and distinct."""
    n = len(seeds)
    e = edges.astype('int64')
    s = np.nonzero(seeds)[0]
    rows = np.concatenate([e[:, 0], np.full(len(s), n)])
    cols = np.concatenate([e[:, 1], s])
    data = np.concatenate([weights, np.full(len(s), weights.min() / 2)])
    forest = minimum_spanning_tree(coo_matrix((data, (rows, cols)), shape=(n + 1, n + 1)).tocsr()).tocoo()
    inner = (forest.row < n) & (forest.col < n)
    g = coo_matrix((np.ones(int(inner.sum())), (forest.row[inner], forest.col[inner])), shape=(n, n))
    comp = connected_components(g, directed=False)[1]
    label_of = np.zeros(int(comp.max()) + 1, dtype='uint64')
    assert len(np.unique(comp[s])) == len(s)  # one seed per tree
    label_of[comp[s]] = seeds[s]
    return label_of[comp]


@pytest.mark.parametrize('seed', range(8))
def test_flood_equals_mst_on_distinct_weights(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(2, 400))
    edges = R.random_graph(rng, n, int(rng.integers(1, 3 * n)))
    weights = 1. + rng.permutation(len(edges)) / len(edges)
    seeds = R.random_seeds(rng, n, int(rng.integers(1, max(2, n // 5))), 4)
    want = _mst_labels(edges, weights, seeds)
    assert np.array_equal(R.flood(edges, weights, seeds), want)
    assert np.array_equal(R.boruvka(edges, weights, seeds), want)


def test_flood_equals_boruvka_where_ties_decide():
    rng = np.random.default_rng(0)
    most_rounds = 0
    for t in range(300):
        n = int(rng.integers(2, 40))
        edges = R.random_graph(rng, n, int(rng.integers(1, 4 * n)))
        if len(edges) == 0:
            continue
        weights = rng.integers(0, 4, len(edges)).astype(float) if t % 2 else rng.random(len(edges))
        seeds = np.where(rng.random(n) < 0.3, rng.integers(1, 4, n), 0).astype('uint64')
        got, rounds = R.boruvka(edges, weights, seeds, return_rounds=True)
        assert np.array_equal(R.flood(edges, weights, seeds), got), t
        most_rounds = max(most_rounds, rounds)
    assert most_rounds >= 2
    # a larger graph with four weight values
    edges, n = R.grid_graph(12)
    weights = rng.integers(0, 4, len(edges)) / 4.
    seeds = R.random_seeds(rng, n, 20, 5)
    assert np.array_equal(R.flood(edges, weights, seeds), R.boruvka(edges, weights, seeds))


def test_flood_small_cases():
    edges, n = R.path_graph(4)
    # ties go to the smaller edge index: edge 0 is popped first and queues edge 1 ahead of edge 2
    assert R.flood(edges, [1., 1., 1.], [5, 0, 0, 9]).tolist() == [5, 5, 5, 9]
    assert R.flood(edges, [1., 1., 0.5], [5, 0, 0, 9]).tolist() == [5, 5, 9, 9]
    assert R.flood(edges, [0., 3., -0.], [5, 0, 0, 9]).tolist() == [5, 5, 9, 9]
    assert R.flood(edges, [1., 1., 1.], [0, 0, 0, 0]).tolist() == [0, 0, 0, 0]
    assert R.flood(edges, [1., 1., 1.], [1, 2, 3, 4]).tolist() == [1, 2, 3, 4]
    assert R.flood(edges[:1], [1.], [0, 2, 0, 0]).tolist() == [2, 2, 0, 0]
    assert R.flood(edges, [1., 1. + 2. ** -40, 1.], [0, 0, 0, 7]).tolist() == [7, 7, 7, 7]
    assert R.flood(edges, [1. + 2. ** -40, 5., 1.], [3, 0, 0, 7]).tolist() == [3, 3, 7, 7]
    with pytest.raises(ValueError):
        R.flood(edges, [1., np.nan, 1.], [1, 0, 0, 0])
    with pytest.raises(ValueError):
        R.flood(edges, [1., 1., 1.], [1, 0, 0])


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_costs_to_weights_equals_the_reference_lines(dtype):
    rng = np.random.default_rng(3)
    costs = (rng.normal(size=5000) * 3).astype(dtype)
    features = costs.copy()
    minc = features.min()
    features -= minc
    features /= features.max()
    features = 1. - features
    got = gws.costs_to_weights(costs)
    assert got.dtype == np.dtype(dtype) and np.array_equal(got, features)
    assert np.array_equal(R.costs_to_weights(costs), features)
    assert got.min() == 0. and got.max() == 1.
    before = costs.copy()
    gws.costs_to_weights(costs)
    assert np.array_equal(costs, before)  # the input is left alone


def test_relabel_first_appearance():
    rng = np.random.default_rng(4)
    labels = rng.integers(0, 50, 2000).astype('uint64') * np.uint64(2 ** 40 + 1)
    got = gws.relabel_first_appearance(labels)
    assert got.dtype == np.uint64 and np.array_equal(got, R.first_appearance(labels))
    assert gws.relabel_first_appearance(np.array([9, 0, 4, 9, 4, 2], dtype='uint64')).tolist() == [1, 0, 2, 1, 2, 3]
    assert gws.relabel_first_appearance(np.zeros(0, dtype='uint64')).tolist() == []


def test_task_seed_steps():
    assignments = np.array([3, 0, 5, 5, 2, 0, 3], dtype='uint64')
    seeds, offset = R.task_seeds(assignments, np.array([5, 2], dtype='uint64'))
    assert offset == 6 and seeds.tolist() == [3, 6, 0, 0, 0, 6, 3]
    with pytest.raises(AssertionError):
        R.task_seeds(assignments, np.array([0, 5]))
    edges, _ = R.path_graph(7)
    weights = np.array([.5, .1, .9, .2, .3, .4])
    assert R.task_result(edges, weights, assignments, [5, 2]).tolist() == [3, 0, 0, 0, 0, 0, 3]
    assert R.task_result(edges, weights, assignments, [5, 2], relabel=True).tolist() == [1, 0, 0, 0, 0, 0, 1]
    # as costs the order turns round (the heaviest cost is the lightest weight): node 2 goes to
    # segment 0 over the cost 0.1, or to segment 2 over the cost 0.9
    assert R.task_result(edges, weights, assignments, [5]).tolist() == [3, 0, 0, 2, 2, 0, 3]
    assert R.task_result(edges, weights, assignments, [5], from_costs=True).tolist() == [3, 0, 2, 2, 2, 0, 3]
