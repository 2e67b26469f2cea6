"""Throughput of the boundary-map edge features of a block (ctws_edge_features_block,
k_edgefeat.hip) on one MI355X, next to ctws_rag_block on the same blocks in the same run and the
numpy restatement (tests/edge_features_ref.py) on one CPU core.

Workload: 64 x 512 x 512 blocks of synthetic DT-watershed fragments with the synthetic boundary
map they came from (float32), core box = the whole block, one block and 16 (the entry point takes
one block: 16 calls), HBM-resident (torch tensors, ctws_edge_features_block_device; the sub-graph
from ctws_rag_block_device stays in HBM) and through host pointers (numpy in / out, PCIe
included).  Times are host clocks around calls that return after the stream has drained; warm-up
calls first.  The stage split is the library's own event timing of the last device call
(Handle.timings(); a stage's span includes its host round trips -- kernel times proper come from a
kernel trace of this script, --device-only).  The sample kernel's rate is given as bytes of a 12 B
per voxel stream over its span.  One JSON line per configuration on stdout.
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

SHAPE = (64, 512, 512)


def make_blocks(h, n_distinct, device):
    from cluster_tools_amd.synthetic import boundary_map_torch
    cfg = dict(size_filter=25, apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=2.0)
    blocks = []
    for k in range(n_distinct):
        x = np.ascontiguousarray(boundary_map_torch(SHAPE, seed=50 + k, device=device).cpu().numpy(), dtype=np.float32)
        blocks.append((h.ws_blocks(cfg, SHAPE, [dict(input=x, block_id=k + 1)])[0]['output'], x))
    return blocks


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--distinct', type=int, default=2, help='distinct blocks the batch cycles through')
    ap.add_argument('--device-only', action='store_true', help='HBM-resident calls only (for a kernel trace)')
    ap.add_argument('--no-numpy', action='store_true', help='skip the restatement on one core')
    args = ap.parse_args()
    import torch
    from cluster_tools_amd import ctws
    dev = torch.device('cuda', 0)
    h = ctws.Handle(0)
    distinct = make_blocks(h, args.distinct, dev)
    n_vox1 = int(np.prod(SHAPE))
    for nb in (1, args.batch):
        src = [distinct[i % len(distinct)] for i in range(nb)]
        dev_lab = [torch.from_numpy(lab.view(np.int64)).to(dev) for lab, _ in src]
        dev_data = [torch.from_numpy(x).to(dev) for _, x in src]
        n_vox = nb * n_vox1
        rec = {'blocks': nb, 'shape': list(SHAPE)}

        t, graphs = timed(lambda: [h.rag_block_device(b, True) for b in dev_lab], args.warmup, args.reps)
        rec.update(rag_device_ms=round(t * 1e3, 3), rag_device_gvox_s=round(n_vox / t / 1e9, 3))
        graphs = [(n.contiguous(), e.contiguous()) for n, e, _ in graphs]

        def run_device():
            return [h.edge_features_block_device(lab, x, n, e, True)
                    for lab, x, (n, e) in zip(dev_lab, dev_data, graphs)]
        t, res = timed(run_device, args.warmup, args.reps)
        tm = h.timings()
        rec.update(edges_per_block=[int(len(r[0])) for r in res[:len(distinct)]],
                   pairs_per_voxel=round(float(res[0][0][:, 9].sum().item()) / n_vox1, 4),
                   n_missing=int(sum(r[1] for r in res)),
                   device_ms=round(t * 1e3, 3), device_gvox_s=round(n_vox / t / 1e9, 3),
                   stages_ms_last_block={k: round(v, 4) for k, v in tm.items()})
        if 'ef_samples' in tm:
            rec['sample_stage_stream_tb_s'] = round(n_vox1 * 12 / (tm['ef_samples'] * 1e-3) / 1e12, 3)
        new_dev = [r[0].cpu().numpy() for r in res]
        if args.device_only:
            print(json.dumps(rec), flush=True)
            continue

        host_graphs = [tuple(a.cpu().numpy().view(np.uint64) for a in g) for g in graphs]
        t, _ = timed(lambda: [h.rag_block(lab, True) for lab, _ in src], 1, max(1, args.reps // 2))
        rec.update(rag_host_ms=round(t * 1e3, 2), rag_host_gvox_s=round(n_vox / t / 1e9, 3))
        t, res = timed(lambda: [h.edge_features_block(lab, x, n, e, True)
                                for (lab, x), (n, e) in zip(src, host_graphs)], 1, max(1, args.reps // 2))
        rec.update(host_ms=round(t * 1e3, 2), host_gvox_s=round(n_vox / t / 1e9, 3))
        rec['same_result'] = bool(all(np.array_equal(a, b[0]) for a, b in zip(new_dev, res)))
        if nb == 1 and not args.no_numpy:
            import edge_features_ref as E
            t0 = time.perf_counter()
            ref, _ = E.block_features(src[0][0], src[0][1], host_graphs[0][1], True)
            t = time.perf_counter() - t0
            rec.update(numpy_one_core_ms=round(t * 1e3, 1), numpy_one_core_gvox_s=round(n_vox1 / t / 1e9, 4))
            rec['max_abs_dev_from_numpy'] = float(np.abs(new_dev[0] - ref).max())
            rec['exact_columns_equal'] = bool(all(np.array_equal(new_dev[0][:, c], ref[:, c]) for c in (9, 2, 8)))
        print(json.dumps(rec), flush=True)
    h.close()


if __name__ == '__main__':
    main()
