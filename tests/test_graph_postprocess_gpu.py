"""Handle.graph_components and Handle.graph_watershed (k_graphpost.hip) against the restatement
(tests/graph_postprocess_ref.py, checked against scipy's csgraph on the CPU).  Both results are
integer arrays with one right answer, so every comparison is exact.  The graphs: a 32^3 grid (more
than one workgroup per kernel, several rounds), the same grid with four weight values (ties decide
most of it), a path of 5,000 nodes with increasing weights (one round whose hook chain has 4,999
links: the deepest pointer jumping), a star with a hub of degree 10,000 (the most contended atomic),
seedless components and isolated nodes; weights that only float64 tells apart, signed zeros and
negative weights; no seed, no unlabelled node, no edge; relabel, float32 weights, device tensors,
repeated calls and the refusals."""
import numpy as np
import pytest

from cluster_tools_amd import ctws
import graph_postprocess_ref as R

pytestmark = pytest.mark.gpu

BIG = np.uint64(2 ** 63 + 11)  # labels are 64-bit


def check_ws(h, edges, weights, seeds, relabel=False):
    got = h.graph_watershed(edges, weights, seeds, relabel)
    want = R.flood(edges, weights, seeds)
    if relabel:
        want = R.first_appearance(want)
    assert got.dtype == np.uint64 and got.shape == (len(seeds),)
    np.testing.assert_array_equal(got, want)
    return got


def check_cc(h, edges, assignments):
    got = h.graph_components(edges, assignments)
    assert got.dtype == np.uint64 and got.shape == (len(assignments),)
    np.testing.assert_array_equal(got, R.components(edges, assignments))
    return got


@pytest.fixture(scope='module')
def grid():
    edges, n = R.grid_graph(32)
    assert n == 32768 and len(edges) == 95232
    rng = np.random.default_rng(7)
    seeds200 = R.random_seeds(rng, n, 200, 5) * BIG
    return dict(edges=edges, n=n, weights=rng.random(len(edges)), ties=rng.integers(0, 4, len(edges)) / 4.,
                seeds200=seeds200, rng=rng)


def test_grid_one_seed(gpu_handle, grid):
    seeds = np.zeros(grid['n'], dtype='uint64')
    seeds[12345] = 3
    got = check_ws(gpu_handle, grid['edges'], grid['weights'], seeds)
    assert (got == 3).all()
    assert gpu_handle.timings()['gw_rounds'] >= 2


def test_grid_200_seeds_of_5_labels(gpu_handle, grid):
    got = check_ws(gpu_handle, grid['edges'], grid['weights'], grid['seeds200'])
    assert len(np.unique(got)) == 5 and (got != 0).all()
    t = gpu_handle.timings()
    assert 2 <= t['gw_rounds'] <= 16 and t['gw_jump_passes'] >= t['gw_rounds']


def test_grid_ties_decide(gpu_handle, grid):
    got = check_ws(gpu_handle, grid['edges'], grid['ties'], grid['seeds200'])
    # the edge order matters here: the same weights on the reversed table give other labels
    rev = R.flood(grid['edges'][::-1], grid['ties'][::-1], grid['seeds200'])
    assert not np.array_equal(got, rev)
    np.testing.assert_array_equal(gpu_handle.graph_watershed(grid['edges'][::-1], grid['ties'][::-1], grid['seeds200']),
                                  rev)


@pytest.mark.parametrize('seed_at,rounds', [(0, 1), (4999, 2)])
def test_path_with_increasing_weights(gpu_handle, seed_at, rounds):
    """Every node's lighter edge leads to its predecessor.  Seed at the light end: one round, a hook
    chain over the whole path.  Seed at the heavy end: the chain first hangs under node 0 (nodes 0
    and 1 choose the same edge, the smaller id stays root), and a second round joins it to the seed."""
    edges, n = R.path_graph(5000)
    seeds = np.zeros(n, dtype='uint64')
    seeds[seed_at] = 9
    got = check_ws(gpu_handle, edges, np.arange(1, n, dtype='float64'), seeds)
    assert (got == 9).all()
    t = gpu_handle.timings()
    assert t['gw_rounds'] == rounds
    assert 1 <= t['gw_jump_passes'] <= 14  # a pass at least halves the depth: 13 for 4,999, and 1 for the second round


@pytest.mark.parametrize('seed_at', [0, 77])
def test_star(gpu_handle, seed_at):
    edges, n = R.star_graph(10000)
    seeds = np.zeros(n, dtype='uint64')
    seeds[seed_at] = 4
    weights = np.random.default_rng(1).random(len(edges))
    assert (check_ws(gpu_handle, edges, weights, seeds) == 4).all()
    weights[:] = 2.5  # every offer to the hub ties
    assert (check_ws(gpu_handle, edges, weights, seeds) == 4).all()


def _parts(rng):
    """Two random parts (nodes 0..299 seeded, 300..499 seedless) and the isolated nodes 500..519,
    one of them a seed."""
    a = R.random_graph(rng, 300, 700)
    b = R.random_graph(rng, 200, 400) + np.uint64(300)
    edges = np.concatenate([a, b])
    edges = edges[rng.permutation(len(edges))]
    seeds = np.zeros(520, dtype='uint64')
    seeds[:300] = R.random_seeds(rng, 300, 12, 6)
    seeds[510] = 8
    return edges, seeds


def test_seedless_component_and_isolated_nodes(gpu_handle):
    rng = np.random.default_rng(2)
    edges, seeds = _parts(rng)
    got = check_ws(gpu_handle, edges, rng.random(len(edges)), seeds)
    assert (got[300:510] == 0).all() and got[510] == 8 and (got[511:] == 0).all() and (got[:300] != 0).any()
    got = check_ws(gpu_handle, edges, rng.integers(0, 3, len(edges)).astype(float), seeds, relabel=True)
    assert (got[300:510] == 0).all() and got.max() <= 7


def test_the_order_is_float64s(gpu_handle):
    edges, _ = R.path_graph(3)
    seeds = np.array([1, 0, 2], dtype='uint64')
    eps = 2. ** -40  # (lost in float32)
    assert check_ws(gpu_handle, edges, [1. + eps, 1.], seeds).tolist() == [1, 2, 2]
    assert check_ws(gpu_handle, edges, [1., 1. + eps], seeds).tolist() == [1, 1, 2]
    assert check_ws(gpu_handle, edges, [-1., -1. - eps], seeds).tolist() == [1, 2, 2]
    assert check_ws(gpu_handle, edges, [5e-324, 0.], seeds).tolist() == [1, 2, 2]
    assert check_ws(gpu_handle, edges, [np.inf, 1e308], seeds).tolist() == [1, 2, 2]
    assert check_ws(gpu_handle, edges, [-1e308, -np.inf], seeds).tolist() == [1, 2, 2]


def test_signed_zeros_tie(gpu_handle):
    edges, _ = R.path_graph(3)
    seeds = np.array([1, 0, 2], dtype='uint64')
    assert check_ws(gpu_handle, edges, [0., -0.], seeds).tolist() == [1, 1, 2]
    assert check_ws(gpu_handle, edges, [-0., 0.], seeds).tolist() == [1, 1, 2]
    assert check_ws(gpu_handle, edges, [0., -5e-324], seeds).tolist() == [1, 2, 2]


def test_negative_weights(gpu_handle):
    rng = np.random.default_rng(3)
    edges, n = R.grid_graph(12)
    seeds = R.random_seeds(rng, n, 30, 30)
    check_ws(gpu_handle, edges, rng.normal(size=len(edges)), seeds)
    check_ws(gpu_handle, edges, -rng.integers(0, 3, len(edges)).astype(float), seeds)


def test_no_seed_and_no_unlabelled_node(gpu_handle):
    rng = np.random.default_rng(4)
    edges = R.random_graph(rng, 1000, 3000)
    weights = rng.random(len(edges))
    assert not check_ws(gpu_handle, edges, weights, np.zeros(1000, dtype='uint64')).any()
    assert gpu_handle.timings()['gw_rounds'] >= 1  # (the seedless components still merge)
    seeds = rng.integers(1, 50, 1000).astype('uint64') * BIG
    np.testing.assert_array_equal(check_ws(gpu_handle, edges, weights, seeds), seeds)
    assert gpu_handle.timings()['gw_rounds'] == 0


def test_no_edge(gpu_handle):
    seeds = np.array([0, 4, 4, 0, 9, 4], dtype='uint64')
    none = np.zeros((0, 2), dtype='uint64')
    assert check_ws(gpu_handle, none, [], seeds).tolist() == seeds.tolist()
    assert check_ws(gpu_handle, none, [], seeds, relabel=True).tolist() == [0, 1, 1, 0, 2, 1]
    assert check_cc(gpu_handle, none, seeds).tolist() == [0, 1, 2, 0, 3, 4]
    assert gpu_handle.graph_watershed(none, [], []).shape == (0,)
    assert gpu_handle.graph_components(none, []).shape == (0,)


def test_relabel(gpu_handle, grid):
    got = check_ws(gpu_handle, grid['edges'], grid['weights'], grid['seeds200'], relabel=True)
    assert sorted(np.unique(got)) == [1, 2, 3, 4, 5] and got[0] == 1
    rng = np.random.default_rng(5)
    seeds = R.random_seeds(rng, grid['n'], 3000, 1500) * np.uint64(0x9E3779B97F4A7C15)  # (wraps: scattered 64-bit labels)
    seeds[rng.random(grid['n']) < 0.001] = 0
    check_ws(gpu_handle, grid['edges'], grid['ties'], seeds, relabel=True)


def test_float32_weights(gpu_handle, grid):
    w32 = grid['weights'].astype('float32')
    got = gpu_handle.graph_watershed(grid['edges'], w32, grid['seeds200'])
    np.testing.assert_array_equal(got, R.flood(grid['edges'], w32.astype('float64'), grid['seeds200']))


def test_device_tensors(gpu_handle, grid):
    import torch
    dev = torch.device('cuda', gpu_handle.device)
    edges = torch.from_numpy(grid['edges'].view(np.int64)).to(dev)
    seeds = torch.from_numpy(grid['seeds200'].view(np.int64)).to(dev)
    host = gpu_handle.graph_watershed(grid['edges'], grid['ties'], grid['seeds200'])
    for dtype in (torch.float64, torch.float32):
        weights = torch.from_numpy(grid['ties']).to(dev).to(dtype)
        for relabel in (False, True):
            got = gpu_handle.graph_watershed_device(edges, weights, seeds, relabel)
            assert got.is_cuda and got.dtype == torch.int64
            want = R.first_appearance(host) if relabel else host
            np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), want)
    np.testing.assert_array_equal(seeds.cpu().numpy().view(np.uint64), grid['seeds200'])  # inputs are left alone
    assignments = (1 + np.arange(grid['n']) % 5).astype('uint64')
    got = gpu_handle.graph_components_device(edges, torch.from_numpy(assignments.view(np.int64)).to(dev))
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), gpu_handle.graph_components(grid['edges'], assignments))
    none = torch.zeros((0, 2), dtype=torch.int64, device=dev)
    got = gpu_handle.graph_watershed_device(none, torch.zeros(0, dtype=torch.float64, device=dev), seeds)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), grid['seeds200'])


def test_repeated_calls_give_equal_bytes(gpu_handle, grid):
    ws = [gpu_handle.graph_watershed(grid['edges'], grid['ties'], grid['seeds200']).tobytes() for _ in range(3)]
    assert ws[0] == ws[1] == ws[2]
    assignments = (1 + np.arange(grid['n']) % 5).astype('uint64')
    cc = [gpu_handle.graph_components(grid['edges'], assignments).tobytes() for _ in range(3)]
    assert cc[0] == cc[1] == cc[2]


def test_refusals(gpu_handle):
    edges, n = R.path_graph(100)
    weights = np.arange(99, dtype='float64')
    seeds = np.zeros(n, dtype='uint64')
    seeds[50] = 1
    with pytest.raises(ctws.CtwsError, match='id >= n_nodes'):
        gpu_handle.graph_watershed(edges, weights, seeds[:99])
    with pytest.raises(ctws.CtwsError, match='id >= n_nodes'):
        gpu_handle.graph_components(edges, seeds[:99])
    with pytest.raises(ctws.CtwsError, match='id >= n_nodes'):
        gpu_handle.graph_components(np.array([[0, 2 ** 40]], dtype='uint64'), seeds)
    with pytest.raises(ctws.CtwsError, match='id >= n_nodes'):
        gpu_handle.graph_watershed(edges[:1], [1.], [])
    bad = weights.copy()
    bad[17] = np.nan
    with pytest.raises(ctws.CtwsError, match='1 weights are NaN'):
        gpu_handle.graph_watershed(edges, bad, seeds)
    with pytest.raises(ValueError, match='98 weights for 99 edges'):
        gpu_handle.graph_watershed(edges, weights[:98], seeds)
    # the handle goes on working
    assert (check_ws(gpu_handle, edges, weights, seeds) == 1).all()


@pytest.mark.parametrize('graph', ['grid', 'path', 'star', 'parts'])
def test_components(gpu_handle, grid, graph):
    rng = np.random.default_rng(6)
    if graph == 'grid':
        edges, n = grid['edges'], grid['n']
    elif graph == 'path':
        edges, n = R.path_graph(5000)
    elif graph == 'star':
        edges, n = R.star_graph(10000)
    else:
        edges, n = _parts(rng)[0], 520
    ids = np.arange(n)
    got = check_cc(gpu_handle, edges, (1 + ids % 5).astype('uint64') * BIG)  # disconnected segments
    assert got.max() > 5 and got[0] == 1
    got = check_cc(gpu_handle, edges, rng.integers(0, 3, n).astype('uint64'))  # with zeros
    assert (got == 0).any()
    got = check_cc(gpu_handle, edges, np.full(n, 7, dtype='uint64'))  # all equal: the graph's own components
    assert (got == 1).all() if graph != 'parts' else got.max() > 20
    got = check_cc(gpu_handle, edges, (1 + ids[::-1]).astype('uint64'))  # all distinct: every node its own
    np.testing.assert_array_equal(got, 1 + ids)
    # the order of the rows and of their ends does not matter
    shuffled = edges[rng.permutation(len(edges))][:, ::-1]
    np.testing.assert_array_equal(gpu_handle.graph_components(shuffled, (1 + ids % 5).astype('uint64')),
                                  R.components(edges, (1 + ids % 5).astype('uint64')))
