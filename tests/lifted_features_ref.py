"""Restatement of the lifted-feature semantics in numpy: what the GPU call
and the tasks of cluster_tools_amd/lifted_features are compared against.  nifty is not available,
so `ndist.computeLiftedNeighborhoodFromNodeLabels` is decided here, not reproduced.

  lifted_neighborhood   a bounded breadth-first search from every labelled node over a CSR of both
                        directions of the edge table
  lifted_costs          costs_from_node_labels.py:119-138
  clear_lifted_edges    clear_lifted_edges_from_labels.py:110-126
"""
import numpy as np

MODES = ('all', 'same', 'different')


def check_edges(edges, n_nodes):
    """The edge table of graph/serialization.py: (m, 2) uint64, u < v, rows strictly ascending,
    every id below n_nodes."""
    edges = np.asarray(edges, dtype='uint64').reshape(-1, 2)
    if len(edges):
        if int(edges.max()) >= n_nodes:
            raise ValueError("an id >= n_nodes")
        if not (edges[:, 0] < edges[:, 1]).all():
            raise ValueError("a row with u >= v")
        a, b = edges[:-1], edges[1:]
        if not ((a[:, 0] < b[:, 0]) | ((a[:, 0] == b[:, 0]) & (a[:, 1] < b[:, 1]))).all():
            raise ValueError("rows not sorted or not unique")
    return edges


def csr(edges, n_nodes):
    """(indptr (n + 1), indices (2 m)) of both directions, int64."""
    e = edges.astype('int64')
    heads = np.concatenate([e[:, 0], e[:, 1]])
    tails = np.concatenate([e[:, 1], e[:, 0]])
    order = np.argsort(heads, kind='stable')
    indptr = np.zeros(n_nodes + 1, dtype='int64')
    np.cumsum(np.bincount(heads, minlength=n_nodes), out=indptr[1:])
    return indptr, tails[order]


def _neighbours(indptr, indices, frontier):
    starts = indptr[frontier]
    lens = indptr[frontier + 1] - starts
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, dtype='int64')
    first = np.cumsum(lens) - lens  # of every list in the gathered array
    return indices[np.repeat(starts - first, lens) + np.arange(total)]


def lifted_neighborhood(edges, node_labels, depth, mode='all', ignore_label=0, return_visits=False):
    """The lifted edge set, (k, 2) uint64 in the order of np.unique(axis=0): all (u, v) with u < v,
    both labels != ignore_label, hop distance 2 <= d(u, v) <= depth in the whole graph, and equal
    ('same'), unequal ('different') or any ('all') labels.  return_visits: also the adjacency
    entries the searches looked at."""
    if mode not in MODES:
        raise ValueError("unknown mode %r" % (mode,))
    if int(depth) != depth or depth < 1:
        raise ValueError("depth >= 1")
    labels = np.asarray(node_labels, dtype='uint64').ravel()
    n = len(labels)
    edges = check_edges(edges, n)
    rows, visits = [], 0
    if len(edges):
        indptr, indices = csr(edges, n)
        labelled = labels != np.uint64(int(ignore_label) & 0xFFFFFFFFFFFFFFFF)
        visited = np.zeros(n, dtype=bool)
        for u in np.flatnonzero(labelled):
            frontier = np.array([u], dtype='int64')
            seen = [frontier]
            visited[u] = True
            for level in range(1, int(depth) + 1):
                nb = _neighbours(indptr, indices, frontier)
                visits += len(nb)
                nb = np.unique(nb)
                nb = nb[~visited[nb]]
                if not len(nb):
                    break
                visited[nb] = True
                seen.append(nb)
                if level >= 2:
                    cand = nb[(nb > u) & labelled[nb]]
                    if mode == 'same':
                        cand = cand[labels[cand] == labels[u]]
                    elif mode == 'different':
                        cand = cand[labels[cand] != labels[u]]
                    if len(cand):
                        rows.append(np.stack([np.full(len(cand), u, dtype='int64'), cand], axis=1))
                frontier = nb
            visited[np.concatenate(seen)] = False
    out = np.concatenate(rows).astype('uint64') if rows else np.zeros((0, 2), dtype='uint64')
    # (the sources ascend and every source's rows ascend level by level only: sort)
    out = out[np.lexsort((out[:, 1], out[:, 0]))]
    return (out, visits) if return_visits else out


def lifted_costs(lifted_edges, node_labels, intra_label_cost=6., inter_label_cost=-6.):
    """float32 (k,): intra_label_cost where the two node labels are equal, else inter_label_cost;
    an endpoint with label 0 is an error."""
    labels = np.asarray(node_labels)
    uv = np.asarray(lifted_edges, dtype='uint64').reshape(-1, 2).astype('int64')
    la, lb = labels[uv[:, 0]], labels[uv[:, 1]]
    if (la == 0).any() or (lb == 0).any():
        raise ValueError("a lifted edge with an unlabelled endpoint")
    costs = np.full(len(uv), intra_label_cost, dtype='float32')
    costs[la != lb] = inter_label_cost
    return costs


def clear_lifted_edges(lifted_edges, clear_labels):
    """The lifted edges whose endpoints have equal labels in the second node labelling."""
    uv = np.asarray(lifted_edges, dtype='uint64').reshape(-1, 2)
    mapped = np.asarray(clear_labels)[uv.astype('int64')]
    return uv[mapped[:, 0] == mapped[:, 1]]


# ---- the graphs the tests and the benchmark share ------------------------------------------

def sort_edges(edges):
    edges = np.asarray(edges, dtype='uint64').reshape(-1, 2)
    return edges[np.lexsort((edges[:, 1], edges[:, 0]))]


def grid_graph(side):
    """A side^3 grid with the 6-neighbourhood, node id = 1 + C-order index, node 0 isolated:
    (edges sorted, n_nodes).  Labels: grid_labels."""
    idx = np.arange(side ** 3, dtype='uint64').reshape(side, side, side) + np.uint64(1)
    pairs = []
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, side - 1), slice(1, side)
        pairs.append(np.stack([idx[tuple(lo)].ravel(), idx[tuple(hi)].ravel()], axis=1))
    return sort_edges(np.concatenate(pairs)), side ** 3 + 1


def grid_labels(n_nodes):
    """labels[k] = k % 5 + 1 where k % 3 == 1, else 0."""
    k = np.arange(n_nodes)
    return np.where(k % 3 == 1, k % 5 + 1, 0).astype('uint64')


def star_graph(n_leaves):
    """Hub 0 unlabelled, leaves 1 .. n_leaves with label 1: (edges, labels)."""
    leaves = np.arange(1, n_leaves + 1, dtype='uint64')
    labels = np.ones(n_leaves + 1, dtype='uint64')
    labels[0] = 0
    return np.stack([np.zeros(n_leaves, dtype='uint64'), leaves], axis=1), labels


def two_level_star(n_middle, n_leaves):
    """Hub 0, n_middle middle nodes with n_leaves leaves each, ids in creation order (a middle
    node, then its leaves): (edges sorted, n_nodes)."""
    rows, nxt = [], 1
    for _ in range(n_middle):
        mid = nxt
        rows.append((0, mid))
        rows.extend((mid, mid + 1 + j) for j in range(n_leaves))
        nxt = mid + 1 + n_leaves
    return sort_edges(np.array(rows, dtype='uint64')), nxt
