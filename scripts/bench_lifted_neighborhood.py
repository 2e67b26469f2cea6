"""Throughput of the sparse lifted neighbourhood (ctws_lifted_neighborhood, k_lifted.hip) on one
MI355X, next to the numpy restatement (tests/lifted_features_ref.py) on one CPU core on the same
input.  nifty is not available: the baseline is the restatement, not
`ndist.computeLiftedNeighborhoodFromNodeLabels`.

Workloads: a side^3 grid graph (6-neighbourhood, node id = 1 + C-order index) with the labelling of
the grid test (labels[k] = k % 5 + 1 where k % 3 == 1, else 0) at depths 2, 3 and 4, mode 'all';
with --rag also the region adjacency graph of 64 x 512 x 512 blocks of synthetic DT-watershed
fragments (Handle.rag_block), node ids = ranks of the fragment ids, the same labelling rule.
HBM-resident (torch tensors, ctws_lifted_neighborhood_device) and through host pointers (numpy in /
out, PCIe included).  Times are host clocks around calls that return after the stream has drained;
warm-up calls first.  The stage split is the library's own event timing of the last device call
(Handle.timings(): lf_csr = degrees, scan and fill; lf_bfs = the search, all its passes; lf_sort =
radix sort and unpack; kernel times proper come from a kernel trace of this script with
--device-only).  Rates: lifted edges per second and adjacency entries visited per second (the
kernel counts them; the restatement counts the same).  One JSON line per configuration on stdout.
"""
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


def rag_graph(h, device, seed):
    """The RAG of one 64 x 512 x 512 block of synthetic fragments with consecutive node ids."""
    from cluster_tools_amd.synthetic import boundary_map_torch
    shape = (64, 512, 512)
    cfg = dict(size_filter=25, apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=2.0)
    x = np.ascontiguousarray(boundary_map_torch(shape, seed=seed, device=device).cpu().numpy(), dtype=np.float32)
    seg = h.ws_blocks(cfg, shape, [dict(input=x, block_id=1)])[0]['output']
    nodes, edges, _ = h.rag_block(seg, True)
    ranks = np.searchsorted(nodes, edges).astype('uint64')  # (sorted rows stay sorted under the ranks)
    return ranks, len(nodes)


def bench(h, dev, name, edges, n_nodes, depths, args):
    import torch
    import lifted_features_ref as R
    labels = R.grid_labels(n_nodes)
    de = torch.from_numpy(edges.view(np.int64)).to(dev)
    dl = torch.from_numpy(labels.view(np.int64)).to(dev)
    for depth in depths:
        rec = {'graph': name, 'n_nodes': int(n_nodes), 'n_edges': int(len(edges)),
               'n_labelled': int((labels != 0).sum()), 'depth': depth, 'mode': 'all'}
        t, out = timed(lambda: h.lifted_neighborhood_device(de, dl, depth), args.warmup, args.reps)
        tm = h.timings()
        k, visits = int(out.shape[0]), float(tm.get('lf_visits', 0.))
        rec.update(lifted_edges=k, adjacency_visits=int(visits), device_ms=round(t * 1e3, 3),
                   device_lifted_edges_per_s=round(k / t, 1), device_visits_per_s=round(visits / t, 1),
                   stages_last_call={key: round(v, 4) for key, v in tm.items()})
        if tm.get('lf_bfs'):
            rec['bfs_stage_visits_per_s'] = round(visits * tm.get('lf_bfs_passes', 1.) / (tm['lf_bfs'] * 1e-3), 1)
        dev_rows = out.cpu().numpy().view(np.uint64)
        if not args.device_only:
            t, host_rows = timed(lambda: h.lifted_neighborhood(edges, labels, depth), 1, max(1, args.reps // 2))
            rec.update(host_ms=round(t * 1e3, 3), host_lifted_edges_per_s=round(k / t, 1),
                       same_result=bool(np.array_equal(dev_rows, host_rows)))
            if not args.no_numpy:
                t0 = time.perf_counter()
                ref, ref_visits = R.lifted_neighborhood(edges, labels, depth, return_visits=True)
                t = time.perf_counter() - t0
                rec.update(numpy_one_core_ms=round(t * 1e3, 1), numpy_lifted_edges_per_s=round(len(ref) / t, 1),
                           numpy_visits_per_s=round(ref_visits / t, 1), numpy_visits=int(ref_visits),
                           equals_numpy=bool(np.array_equal(dev_rows, ref)))
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--side', type=int, default=128, help='the grid graph has side^3 nodes')
    ap.add_argument('--depths', type=int, nargs='+', default=[2, 3, 4])
    ap.add_argument('--rag', action='store_true', help='also the RAG of a block of synthetic fragments')
    ap.add_argument('--device-only', action='store_true', help='HBM-resident calls only (for a kernel trace)')
    ap.add_argument('--no-numpy', action='store_true', help='skip the restatement on one core')
    args = ap.parse_args()
    import torch
    from cluster_tools_amd import ctws
    import lifted_features_ref as R
    dev = torch.device('cuda', 0)
    h = ctws.Handle(0)
    edges, n_nodes = R.grid_graph(args.side)
    bench(h, dev, 'grid_%i' % args.side, edges, n_nodes, args.depths, args)
    if args.rag:
        edges, n_nodes = rag_graph(h, dev, 50)
        bench(h, dev, 'rag_64x512x512', edges, n_nodes, args.depths, args)
    h.close()


if __name__ == '__main__':
    main()
