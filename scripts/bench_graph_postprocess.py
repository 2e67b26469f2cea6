"""Throughput of the graph postprocessing calls (ctws_graph_components, ctws_graph_watershed,
k_graphpost.hip) on one MI355X, next to three baselines on one CPU core on the same input: scipy's
`connected_components`, scipy's `minimum_spanning_tree` on the graph plus a virtual root (compiled
code, the fair CPU figure for the watershed; it computes the forest, not yet the labels), and the
heapq restatement of the flood (tests/graph_postprocess_ref.py).  nifty is not available: its
`connectedComponentsFromNodes` and `edgeWeightedWatershedsSegmentation` are not measured.

Workload: a side^3 grid graph (6-neighbourhood), random float64 weights, 1 % of the nodes seeded
with one of 1000 labels; components on the assignment 1 + (z // 16) of the grid (slabs, so that the
union-find has real work).  HBM-resident (torch tensors, the _device calls) and through host pointers
(numpy in / out, PCIe included).  Times are host clocks around calls that return after the stream
has drained; warm-up calls first.  The stage split is the library's own event timing of the last
device call (Handle.timings(): gw_sort = checks, radix sort, ends in rank order; gw_rounds_ms = the
rounds with their pointer jumping and read-backs; gw_write = labels and relabel); kernel times
proper come from a kernel trace of this script with --device-only.  One JSON line per call on
stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def rates(rec, prefix, t, n, m):
    rec.update({prefix + '_ms': round(t * 1e3, 3), prefix + '_nodes_per_s': round(n / t, 1),
                prefix + '_edges_per_s': round(m / t, 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--side', type=int, default=128, help='the grid graph has side^3 nodes')
    ap.add_argument('--device-only', action='store_true', help='HBM-resident calls only (for a kernel trace)')
    ap.add_argument('--no-heapq', action='store_true', help='skip the heapq restatement on one core')
    args = ap.parse_args()
    import torch
    from cluster_tools_amd import ctws
    import graph_postprocess_ref as R
    dev = torch.device('cuda', 0)
    h = ctws.Handle(0)
    edges, n = R.grid_graph(args.side)
    m = len(edges)
    rng = np.random.default_rng(0)
    weights = rng.random(m)
    seeds = R.random_seeds(rng, n, n // 100, 1000)
    assignments = (1 + np.arange(n) // (16 * args.side * args.side)).astype('uint64')
    base = {'graph': 'grid_%i' % args.side, 'n_nodes': int(n), 'n_edges': int(m)}
    de = torch.from_numpy(edges.view(np.int64)).to(dev)
    dw = torch.from_numpy(weights).to(dev)
    ds = torch.from_numpy(seeds.view(np.int64)).to(dev)
    da = torch.from_numpy(assignments.view(np.int64)).to(dev)

    # ---- components
    rec = dict(base, call='graph_components', n_segments=int(assignments.max()))
    t, out = timed(lambda: h.graph_components_device(de, da), args.warmup, args.reps)
    rates(rec, 'device', t, n, m)
    rec['stages_last_call'] = {k: round(v, 4) for k, v in h.timings().items()}
    cc_dev = out.cpu().numpy().view(np.uint64)
    rec['n_components'] = int(cc_dev.max())
    if not args.device_only:
        t, cc_host = timed(lambda: h.graph_components(edges, assignments), 1, max(1, args.reps // 2))
        rates(rec, 'host', t, n, m)
        rec['same_result'] = bool(np.array_equal(cc_dev, cc_host))
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components, minimum_spanning_tree
        e = edges.astype(np.int64)

        def scipy_cc():
            keep = (assignments[e[:, 0]] == assignments[e[:, 1]]) & (assignments[e[:, 0]] != 0)
            g = coo_matrix((np.ones(int(keep.sum()), dtype=np.int8), (e[keep, 0], e[keep, 1])), shape=(n, n)).tocsr()
            return connected_components(g, directed=False)
        t, (k, _) = once(scipy_cc)
        rates(rec, 'scipy_one_core', t, n, m)
        rec['scipy_n_components'] = int(k)
    print(json.dumps(rec), flush=True)

    # ---- watershed
    for relabel in (False, True):
        rec = dict(base, call='graph_watershed', relabel=relabel, n_seeds=int((seeds != 0).sum()))
        t, out = timed(lambda: h.graph_watershed_device(de, dw, ds, relabel), args.warmup, args.reps)
        rates(rec, 'device', t, n, m)
        tm = h.timings()
        rec['rounds'] = int(tm.get('gw_rounds', -1))
        rec['jump_passes'] = int(tm.get('gw_jump_passes', -1))
        rec['stages_last_call'] = {k: round(v, 4) for k, v in tm.items()}
        ws_dev = out.cpu().numpy().view(np.uint64)
        if not args.device_only:
            t, ws_host = timed(lambda: h.graph_watershed(edges, weights, seeds, relabel), 1, max(1, args.reps // 2))
            rates(rec, 'host', t, n, m)
            rec['same_result'] = bool(np.array_equal(ws_dev, ws_host))
            if not relabel:
                s = np.nonzero(seeds)[0]

                def scipy_mst():
                    rows = np.concatenate([e[:, 0], np.full(len(s), n)])
                    cols = np.concatenate([e[:, 1], s])
                    data = np.concatenate([weights + 1., np.full(len(s), 0.5)])  # (0 is "no edge" to csgraph)
                    return minimum_spanning_tree(coo_matrix((data, (rows, cols)), shape=(n + 1, n + 1)).tocsr())
                t, forest = once(scipy_mst)
                rates(rec, 'scipy_mst_one_core', t, n, m)
                rec['scipy_mst_edges'] = int(forest.nnz)
                if not args.no_heapq:
                    t, ref = once(lambda: R.flood(edges, weights, seeds))
                    rates(rec, 'heapq_one_core', t, n, m)
                    rec['equals_heapq'] = bool(np.array_equal(ws_dev, ref))
        print(json.dumps(rec), flush=True)
    h.close()


if __name__ == '__main__':
    main()
