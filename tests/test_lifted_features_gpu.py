"""Handle.lifted_neighborhood (ctws_lifted_neighborhood, k_lifted.hip) against the numpy restatement
(tests/lifted_features_ref.py): the result is an integer table in a canonical order, so every
comparison is exact.  The graphs are the smallest that reach each path of the search: a frontier
wider than a wave, a second pass at the counted size, two shortest paths to one node, a source whose
reach overflows the on-chip visited set and the list in LDS, 64-bit labels, an ignore label that is
not 0, several components."""
import numpy as np
import pytest

from cluster_tools_amd import ctws
import lifted_features_ref as R

pytestmark = pytest.mark.gpu


def check(h, edges, labels, depth, mode='all', ignore_label=0):
    got = h.lifted_neighborhood(edges, labels, depth, mode, ignore_label)
    want = R.lifted_neighborhood(edges, labels, depth, mode, ignore_label)
    assert got.dtype == np.uint64 and got.ndim == 2 and got.shape[1] == 2
    np.testing.assert_array_equal(got, want)
    return got


def test_path(gpu_handle):
    edges = np.array([[i, i + 1] for i in range(5)], dtype='uint64')
    labels = np.ones(6, dtype='uint64')
    counts = [len(check(gpu_handle, edges, labels, d, ignore_label=7)) for d in range(1, 7)]
    assert counts == [0, 4, 7, 9, 10, 10]


def test_path_through_a_smaller_unlabelled_node(gpu_handle):
    labels = np.zeros(8, dtype='uint64')
    labels[[5, 7]] = 3
    edges = np.array([[0, 5], [0, 7]], dtype='uint64')
    assert check(gpu_handle, edges, labels, 2).tolist() == [[5, 7]]
    assert check(gpu_handle, edges, labels, 2, 'same').tolist() == [[5, 7]]
    assert check(gpu_handle, edges, labels, 2, 'different').shape == (0, 2)


def test_direct_neighbours_are_excluded(gpu_handle):
    edges = np.array([[1, 2], [1, 3], [2, 3], [3, 4]], dtype='uint64')
    labels = np.array([0, 1, 1, 1, 1], dtype='uint64')
    assert check(gpu_handle, edges, labels, 2).tolist() == [[1, 4], [2, 4]]


def test_star(gpu_handle):
    """A frontier wider than a wave, 199 emits from one source."""
    edges, labels = R.star_graph(200)
    assert len(check(gpu_handle, edges, labels, 2)) == 19900
    assert check(gpu_handle, edges, labels, 1).shape == (0, 2)
    assert len(check(gpu_handle, edges, labels, 3, 'same')) == 19900
    assert check(gpu_handle, edges, labels, 3, 'different').shape == (0, 2)


def test_second_pass_at_the_counted_size(gpu_handle):
    """More lifted edges than the first capacity of the key buffer: the search runs twice."""
    n_leaves = 400
    edges, labels = R.star_graph(n_leaves)
    first_cap, _ = ctws.lifted_limits(n_leaves)
    while n_leaves * (n_leaves - 1) // 2 <= first_cap:  # (a larger first capacity: a larger star)
        n_leaves *= 2
        edges, labels = R.star_graph(n_leaves)
        first_cap, _ = ctws.lifted_limits(n_leaves)
    got = check(gpu_handle, edges, labels, 2)
    assert len(got) == n_leaves * (n_leaves - 1) // 2 > first_cap
    t = gpu_handle.timings()
    assert t['lf_bfs_passes'] == 2 and t['lf_keys'] == len(got) and t['lf_sources'] == n_leaves


def test_cycle_two_shortest_paths(gpu_handle):
    edges = R.sort_edges([[i, i + 1] for i in range(8)] + [[0, 8]])
    labels = np.ones(9, dtype='uint64')
    got = check(gpu_handle, edges, labels, 4)
    assert len(got) == 9 * 8 // 2 - 9  # every pair but the 9 edges: the diameter is 4
    assert len(check(gpu_handle, edges, labels, 3)) == 18


@pytest.fixture(scope='module')
def grid():
    edges, n = R.grid_graph(12)
    labels = R.grid_labels(n)
    assert len(edges) == 4752 and n == 1729 and int((labels != 0).sum()) == 576
    return edges, labels


@pytest.mark.parametrize('mode,rows', [('all', 9720), ('same', 2068), ('different', 7652)])
def test_grid(gpu_handle, grid, mode, rows):
    edges, labels = grid
    assert len(check(gpu_handle, edges, labels, 4, mode)) == rows


def test_grid_other_depths(gpu_handle, grid):
    edges, labels = grid
    for depth in (1, 2, 3, 7):
        check(gpu_handle, edges, labels, depth)


def test_reach_overflows_the_visited_set(gpu_handle):
    """Source 2 reaches every node: more than the hash set in LDS takes and more than the part of
    the node list in LDS, so the wave goes on in its bitmap and its global queue; the sources
    behind it on the same wave find the bitmap cleared."""
    _, visited_cap = ctws.lifted_limits(0)
    n_middle, n_leaves = 300, 40
    while n_middle * (n_leaves + 1) + 1 <= 2 * visited_cap:
        n_leaves *= 2
    edges, n = R.two_level_star(n_middle, n_leaves)
    labels = np.zeros(n, dtype='uint64')
    labels[1] = labels[2] = 7
    labels[n - 1] = 9
    assert n > 2 * visited_cap and len(edges) == n - 1
    assert check(gpu_handle, edges, labels, 4).tolist() == [[1, n - 1], [2, n - 1]]
    assert check(gpu_handle, edges, labels, 4, 'same').shape == (0, 2)
    if n_leaves == 40:
        assert n == 12301
    # every node labelled: every source overflows at depth 4, several per wave
    small, ns = R.two_level_star(40, visited_cap // 40 + 2)
    assert ns > visited_cap
    check(gpu_handle, small, (np.arange(ns) % 3 + 1).astype('uint64'), 4, 'same')
    # and with sources that overflow next to sources that do not (depth 3: only the middle nodes,
    # the hub and the leaves' parents reach far)
    sparse = np.zeros(n, dtype='uint64')
    sparse[::29] = 1
    sparse[1] = 2
    check(gpu_handle, edges, sparse, 3)
    check(gpu_handle, edges, sparse, 4, 'different')


def test_labels_above_32_bits(gpu_handle):
    edges = np.array([[i, i + 1] for i in range(7)], dtype='uint64')
    labels = np.array([5, 5 + 2 ** 32, 5, 5 + 2 ** 33, 5 + 2 ** 32, 2 ** 63 + 5, 5, 2 ** 63 + 5], dtype='uint64')
    same = check(gpu_handle, edges, labels, 3, 'same')
    diff = check(gpu_handle, edges, labels, 3, 'different')
    assert same.tolist() == [[0, 2], [1, 4], [5, 7]]
    assert len(same) + len(diff) == len(check(gpu_handle, edges, labels, 3, 'all')) == 11


def test_ignore_label_not_zero(gpu_handle):
    edges = np.array([[i, i + 1] for i in range(6)], dtype='uint64')
    labels = np.array([0, 4, 0, 4, 1, 0, 4], dtype='uint64')
    got = check(gpu_handle, edges, labels, 2, ignore_label=4)  # label 0 is a label here
    assert got.tolist() == [[0, 2], [2, 4]]
    check(gpu_handle, edges, labels, 4, 'same', ignore_label=4)
    check(gpu_handle, edges, labels, 4, 'different', ignore_label=2 ** 64 - 1)  # nothing is ignored


def test_components_and_an_isolated_node(gpu_handle):
    edges = R.sort_edges([[0, 1], [1, 2], [2, 3], [5, 6], [6, 7], [5, 7], [7, 8]])
    labels = np.array([1, 0, 1, 2, 3, 2, 0, 1, 2, 9], dtype='uint64')  # 4 and 9 are isolated
    assert check(gpu_handle, edges, labels, 5).tolist() == [[0, 2], [0, 3], [5, 8]]
    assert check(gpu_handle, edges, labels, 5, 'same').tolist() == [[0, 2], [5, 8]]


def test_repeated_calls_and_device_pointers(gpu_handle, grid):
    import torch
    edges, labels = grid
    first = gpu_handle.lifted_neighborhood(edges, labels, 4, 'different')
    for _ in range(2):
        again = gpu_handle.lifted_neighborhood(edges, labels, 4, 'different')
        assert again.tobytes() == first.tobytes()
    dev = torch.device('cuda', 0)
    de = torch.from_numpy(edges.view(np.int64)).to(dev)
    dl = torch.from_numpy(labels.view(np.int64)).to(dev)
    out = gpu_handle.lifted_neighborhood_device(de, dl, 4, 'different')
    assert out.is_cuda and out.dtype == torch.int64 and tuple(out.shape) == first.shape
    assert out.cpu().numpy().view(np.uint64).tobytes() == first.tobytes()


def test_sized_call_reports_the_count_and_writes_nothing_past_cap(gpu_handle, grid):
    edges, labels = grid
    ret, k, out = gpu_handle.lifted_neighborhood_raw(edges, labels, 4, ctws.LIFTED_MODES['all'], 0, 0)
    assert ret == -1 and k == 9720
    out = None
    ret, k, out = gpu_handle.lifted_neighborhood_raw(edges, labels, 4, ctws.LIFTED_MODES['all'], 0, 9720)
    assert ret == 0 and k == 9720
    np.testing.assert_array_equal(out, R.lifted_neighborhood(edges, labels, 4))


def test_empty_results(gpu_handle):
    labels = np.ones(5, dtype='uint64')
    assert gpu_handle.lifted_neighborhood(np.zeros((0, 2), dtype='uint64'), labels, 3).shape == (0, 2)
    edges = np.array([[0, 1], [1, 2], [2, 4]], dtype='uint64')
    got = gpu_handle.lifted_neighborhood(edges, np.zeros(5, dtype='uint64'), 3)
    assert got.shape == (0, 2) and got.dtype == np.uint64
    assert gpu_handle.lifted_neighborhood(edges, labels, 3, ignore_label=1).shape == (0, 2)
    assert 'lf_bfs' not in gpu_handle.timings()  # no labelled node: no search was launched


@pytest.mark.parametrize('edges', [[[0, 1], [1, 5]], [[0, 1], [3, 2]], [[1, 2], [0, 1]], [[0, 1], [0, 1]]],
                         ids=['id_out_of_range', 'u_above_v', 'reversed_rows', 'duplicate_row'])
def test_bad_edge_tables(gpu_handle, edges):
    labels = np.ones(5, dtype='uint64')
    with pytest.raises(ctws.CtwsError, match='edge table'):
        gpu_handle.lifted_neighborhood(np.array(edges, dtype='uint64'), labels, 2)


def test_bad_depth_and_mode(gpu_handle):
    edges = np.array([[0, 1], [1, 2]], dtype='uint64')
    labels = np.ones(3, dtype='uint64')
    for depth in (0, -1, 1.5):
        with pytest.raises(ValueError, match='depth'):
            gpu_handle.lifted_neighborhood(edges, labels, depth)
    with pytest.raises(ValueError, match='mode'):
        gpu_handle.lifted_neighborhood(edges, labels, 2, 'x')
    # the library refuses them too
    ret, _, _ = gpu_handle.lifted_neighborhood_raw(edges, labels, 0, 0, 0, 4)
    assert ret == -1 and 'depth' in gpu_handle.last_error()
    ret, _, _ = gpu_handle.lifted_neighborhood_raw(edges, labels, 2, 3, 0, 4)
    assert ret == -1 and 'mode' in gpu_handle.last_error()
