"""The restatement of the lifted neighbourhood (tests/lifted_features_ref.py) against a brute force
on small dense graphs, and on the hand-checked graphs that pin the decided semantics (DESIGN.md
section 3.12).  CPU only."""
import numpy as np
import pytest

import lifted_features_ref as R


def brute_force(edges, labels, depth, mode, ignore_label):
    """All-pairs hop distances by repeated boolean matrix products, then the definition."""
    n = len(labels)
    adj = np.zeros((n, n), dtype=bool)
    e = np.asarray(edges, dtype='int64').reshape(-1, 2)
    adj[e[:, 0], e[:, 1]] = adj[e[:, 1], e[:, 0]] = True
    dist = np.full((n, n), -1, dtype='int64')
    dist[np.eye(n, dtype=bool)] = 0
    reach = np.eye(n, dtype=bool)
    for d in range(1, depth + 1):
        nxt = (reach.astype('int64') @ adj.astype('int64')) > 0
        new = nxt & (dist < 0)
        dist[new] = d
        reach = reach | nxt
    rows = []
    for u in range(n):
        for v in range(u + 1, n):
            if labels[u] == ignore_label or labels[v] == ignore_label or not 2 <= dist[u, v] <= depth:
                continue
            if mode == 'same' and labels[u] != labels[v]:
                continue
            if mode == 'different' and labels[u] == labels[v]:
                continue
            rows.append((u, v))
    return np.array(rows, dtype='uint64').reshape(-1, 2)


def random_graph(seed, n, p):
    rng = np.random.RandomState(seed)
    u, v = np.triu_indices(n, 1)
    keep = rng.rand(len(u)) < p
    return np.stack([u[keep], v[keep]], axis=1).astype('uint64'), rng


@pytest.mark.parametrize('seed,n,p', [(0, 40, 0.05), (1, 33, 0.1), (2, 17, 0.3), (3, 40, 0.03)])
@pytest.mark.parametrize('with_unlabelled', [False, True])
def test_restatement_against_brute_force(seed, n, p, with_unlabelled):
    edges, rng = random_graph(seed, n, p)
    labels = rng.randint(1, 4, n).astype('uint64')
    if with_unlabelled:
        labels[rng.rand(n) < 0.4] = 0
    total = 0
    for depth in range(1, 6):
        for mode in R.MODES:
            got = R.lifted_neighborhood(edges, labels, depth, mode)
            want = brute_force(edges, labels, depth, mode, 0)
            np.testing.assert_array_equal(got, want)
            assert got.dtype == np.uint64
            total += len(got)
        assert len(R.lifted_neighborhood(edges, labels, depth, 'same')) + len(
            R.lifted_neighborhood(edges, labels, depth, 'different')) == len(
            R.lifted_neighborhood(edges, labels, depth, 'all'))
    assert total > 0


PATH = np.array([[i, i + 1] for i in range(5)], dtype='uint64')


def test_path_counts():
    labels = np.ones(6, dtype='uint64')
    counts = [len(R.lifted_neighborhood(PATH, labels, d, ignore_label=7)) for d in range(1, 7)]
    assert counts == [0, 4, 7, 9, 10, 10]
    np.testing.assert_array_equal(R.lifted_neighborhood(PATH, labels, 2, ignore_label=7),
                                  [[0, 2], [1, 3], [2, 4], [3, 5]])
    # with ignore_label 1 nothing is labelled
    assert R.lifted_neighborhood(PATH, labels, 4, ignore_label=1).shape == (0, 2)


def test_path_through_a_smaller_unlabelled_node():
    labels = np.zeros(8, dtype='uint64')
    labels[[5, 7]] = 3
    edges = np.array([[0, 5], [0, 7]], dtype='uint64')
    for mode, want in (('all', [[5, 7]]), ('same', [[5, 7]]), ('different', np.zeros((0, 2)))):
        np.testing.assert_array_equal(R.lifted_neighborhood(edges, labels, 2, mode), want)
    assert len(R.lifted_neighborhood(edges, labels, 1)) == 0


def test_direct_neighbours_are_excluded():
    edges = np.array([[1, 2], [1, 3], [2, 3], [3, 4]], dtype='uint64')
    labels = np.array([0, 1, 1, 1, 1], dtype='uint64')
    np.testing.assert_array_equal(R.lifted_neighborhood(edges, labels, 2), [[1, 4], [2, 4]])


def test_visit_count_and_errors():
    labels = np.ones(6, dtype='uint64')
    out, visits = R.lifted_neighborhood(PATH, labels, 1, return_visits=True)
    assert len(out) == 0 and visits == 10  # every list once
    for bad in ([[0, 6]], [[2, 1]], [[1, 2], [0, 1]], [[0, 1], [0, 1]]):
        with pytest.raises(ValueError):
            R.lifted_neighborhood(np.array(bad, dtype='uint64'), labels, 2)
    with pytest.raises(ValueError):
        R.lifted_neighborhood(PATH, labels, 0)
    with pytest.raises(ValueError):
        R.lifted_neighborhood(PATH, labels, 2, 'x')


def test_costs_and_clear_rules():
    labels = np.array([0, 4, 4, 2 ** 40, 2 ** 40 + 2 ** 32], dtype='uint64')
    uv = np.array([[1, 2], [1, 3], [3, 4]], dtype='uint64')
    costs = R.lifted_costs(uv, labels)
    assert costs.dtype == np.float32 and costs.tolist() == [6., -6., -6.]
    assert R.lifted_costs(uv, labels, 1.5, -2.5).tolist() == [1.5, -2.5, -2.5]
    with pytest.raises(ValueError):
        R.lifted_costs(np.array([[0, 2]], dtype='uint64'), labels)
    clear = np.array([9, 1, 1, 1, 2], dtype='uint64')
    np.testing.assert_array_equal(R.clear_lifted_edges(uv, clear), [[1, 2], [1, 3]])
