"""The graph postprocessing restated in numpy / heapq: graph connected
components, the seeded graph watershed as the sequential priority-queue flood, the same watershed as
seeded Boruvka rounds (a second, independent restatement of the same answer), the `from_costs`
weights, and the seed and relabel steps of the GraphWatershedAssignments job.  nifty is not
available: these functions are the semantics the GPU results are compared to, and
tests/test_graph_postprocess_ref.py checks them against scipy's csgraph.  Graph builders for the
tests and the benchmark are at the end."""
import heapq

import numpy as np


def _check(edges, n_nodes):
    edges = np.asarray(edges, dtype='uint64').reshape(-1, 2)
    if len(edges) and int(edges.max()) >= n_nodes:
        raise ValueError("an edge holds an id >= n_nodes (%i)" % n_nodes)
    return edges.astype('int64')


def first_appearance(labels):
    """relabelConsecutive(start_label=1, keep_zeros=True): a plain loop over the node array."""
    number, out = {}, np.zeros(len(labels), dtype='uint64')
    for i, lab in enumerate(np.asarray(labels).tolist()):
        if lab:
            out[i] = number.setdefault(lab, len(number) + 1)
    return out


def components(edges, assignments):
    """Two nodes are joined when an edge connects them and both carry the same non-zero
    assignment; 0 stays 0; the components are numbered from 1 in the order of their smallest node."""
    assignments = np.asarray(assignments, dtype='uint64')
    n = len(assignments)
    edges = _check(edges, n)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    keep = (assignments[edges[:, 0]] == assignments[edges[:, 1]]) & (assignments[edges[:, 0]] != 0)
    for u, v in edges[keep].tolist():
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    roots = np.array([find(x) for x in range(n)], dtype='int64')
    # a node's root is its component's smallest node: the numbering is the first appearance of the roots
    return first_appearance(np.where(assignments != 0, roots + 1, 0))


def _weights(weights, m):
    weights = np.asarray(weights, dtype='float64').ravel()
    if len(weights) != m:
        raise ValueError("%i weights for %i edges" % (len(weights), m))
    if np.isnan(weights).any():
        raise ValueError("NaN weights are refused")
    return weights + 0.  # (-0.0 + 0.0 is 0.0)


def _adjacency(edges, n):
    """CSR over both directions: (row, neighbour, edge index), lists in edge order."""
    m = len(edges)
    ends = np.concatenate([edges[:, 0], edges[:, 1]])
    other = np.concatenate([edges[:, 1], edges[:, 0]])
    eid = np.concatenate([np.arange(m), np.arange(m)])
    order = np.argsort(ends, kind='stable')
    row = np.zeros(n + 1, dtype='int64')
    np.cumsum(np.bincount(ends, minlength=n), out=row[1:])
    return row.tolist(), other[order].tolist(), eid[order].tolist()


def flood(edges, weights, seeds):
    """The sequential flood: every edge between a labelled and an unlabelled node is queued; the
    edge with the smallest (weight, edge index) is popped; if exactly one end is unlabelled it takes
    the other's label and its edges to unlabelled nodes are queued.  Unreached nodes keep 0."""
    seeds = np.asarray(seeds, dtype='uint64')
    n = len(seeds)
    edges = _check(edges, n)
    w = _weights(weights, len(edges)).tolist()
    row, nbr, eid = _adjacency(edges, n)
    lab = seeds.tolist()
    uv = edges.tolist()
    queued = [False] * len(uv)
    pq = []

    def push(x):
        for k in range(row[x], row[x + 1]):
            e = eid[k]
            if lab[nbr[k]] == 0 and not queued[e]:
                queued[e] = True
                heapq.heappush(pq, (w[e], e))
    for x in range(n):
        if lab[x]:
            push(x)
    while pq:
        _, e = heapq.heappop(pq)
        u, v = uv[e]
        if (lab[u] == 0) == (lab[v] == 0):
            continue
        x, src = (u, v) if lab[u] == 0 else (v, u)
        lab[x] = lab[src]
        push(x)
    return np.array(lab, dtype='uint64')


def boruvka(edges, weights, seeds, return_rounds=False):
    """The same labels by seeded Boruvka rounds on the total order (weight, edge index): every
    unseeded component takes its best edge to another component (two seeded ones never join), of two
    unseeded components on one edge the smaller id stays root; until no component hooks.  rounds
    counts the rounds that hooked something."""
    seeds = np.asarray(seeds, dtype='uint64')
    n = len(seeds)
    edges = _check(edges, n)
    m = len(edges)
    w = _weights(weights, m)
    order = np.lexsort((np.arange(m), w))
    su, sv = edges[order, 0], edges[order, 1]
    comp = np.arange(n, dtype='int64')
    seeded = seeds != 0
    rounds = 0
    while m:
        cu, cv = comp[su], comp[sv]
        fu, fv = seeded[cu], seeded[cv]
        live = np.nonzero((cu != cv) & ~(fu & fv))[0]
        best = np.full(n, m, dtype='int64')
        np.minimum.at(best, cu[live][~fu[live]], live[~fu[live]])
        np.minimum.at(best, cv[live][~fv[live]], live[~fv[live]])
        c = np.nonzero(best < m)[0]
        e = best[c]
        o = np.where(cu[e] == c, cv[e], cu[e])
        hook = ~(~seeded[o] & (best[o] == e) & (c < o))
        if not hook.any():
            break
        rounds += 1
        par = np.arange(n, dtype='int64')
        par[c[hook]] = o[hook]
        while True:
            nxt = par[par]
            if np.array_equal(nxt, par):
                break
            par = nxt
        comp = par[comp]
    out = seeds[comp]
    return (out, rounds) if return_rounds else out


def costs_to_weights(features):
    """The reference's from_costs lines (graph_watershed_assignments.py:137-141) on a copy."""
    features = np.array(features)
    minc = features.min()
    features -= minc
    features /= features.max()
    features = 1. - features
    return features


def task_seeds(assignments, discard_ids):
    """-> (seeds, seed_offset): 0 becomes max + 1, nodes of a discarded segment become 0."""
    assignments = np.array(assignments, dtype='uint64')
    discard_ids = np.asarray(discard_ids)
    assert 0 not in discard_ids, "Breaks logic"
    seed_offset = int(assignments.max()) + 1
    assignments[assignments == 0] = seed_offset
    assignments[np.isin(assignments, discard_ids)] = 0
    return assignments, seed_offset


def task_result(edges, features, assignments, discard_ids, relabel=False, from_costs=False):
    """What the GraphWatershedAssignments job writes."""
    if from_costs:
        features = costs_to_weights(features)
    seeds, seed_offset = task_seeds(assignments, discard_ids)
    out = flood(edges, features, seeds)
    out[out == seed_offset] = 0
    return first_appearance(out) if relabel else out


# ---- graphs -----------------------------------------------------------------------------------

def grid_graph(side):
    """The 6-neighbourhood graph of a side^3 grid, node id = C-order index: (edges, n_nodes), rows
    sorted."""
    ids = np.arange(side ** 3, dtype='uint64').reshape(side, side, side)
    rows = [np.stack([ids[:-1].ravel(), ids[1:].ravel()], 1),
            np.stack([ids[:, :-1].ravel(), ids[:, 1:].ravel()], 1),
            np.stack([ids[:, :, :-1].ravel(), ids[:, :, 1:].ravel()], 1)]
    edges = np.concatenate(rows)
    return edges[np.lexsort((edges[:, 1], edges[:, 0]))], side ** 3


def path_graph(n):
    ids = np.arange(n, dtype='uint64')
    return np.stack([ids[:-1], ids[1:]], 1), n


def star_graph(degree):
    """Node 0 is the hub."""
    leaves = np.arange(1, degree + 1, dtype='uint64')
    return np.stack([np.zeros_like(leaves), leaves], 1), degree + 1


def random_graph(rng, n, m):
    """Up to m distinct edges u < v on n nodes."""
    uv = rng.integers(0, n, (m, 2))
    uv = uv[uv[:, 0] != uv[:, 1]]
    return np.unique(np.sort(uv, 1), axis=0).astype('uint64')


def random_seeds(rng, n, n_seeds, n_labels):
    seeds = np.zeros(n, dtype='uint64')
    seeds[rng.choice(n, n_seeds, replace=False)] = rng.integers(1, n_labels + 1, n_seeds).astype('uint64')
    return seeds
