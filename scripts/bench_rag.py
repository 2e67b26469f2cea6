"""Throughput of the region adjacency graph of a block (ctws_rag_block, k_rag.hip) on one MI355X,
next to the numpy restatement on one CPU core.

Workload: 64 x 512 x 512 blocks of synthetic DT-watershed fragments (the GPU watershed of the
synthetic boundary map, ids block_id * prod(shape) + k as a WatershedWorkflow leaves them), one
block and 16 (the entry point takes one block: 16 calls), HBM-resident (torch tensors,
ctws_rag_block_device) and through host pointers (numpy in / out, PCIe included).  Times are
host clocks around calls that return after the stream has drained; warm-up calls first.  The
stage split is the library's own event timing of the last device call (Handle.timings(); a
stage's span includes its host round trips -- kernel times proper come from a kernel trace of
this script, --device-only).  The pair kernel's rate is given as bytes of an 8 B per voxel stream
over its span.  One JSON line per configuration on stdout.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPE = (64, 512, 512)


def make_blocks(h, n_distinct, device):
    from cluster_tools_amd.synthetic import boundary_map_torch
    cfg = dict(size_filter=25, apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=2.0)
    blocks = []
    for k in range(n_distinct):
        x = boundary_map_torch(SHAPE, seed=50 + k, device=device).cpu().numpy()
        blocks.append(h.ws_blocks(cfg, SHAPE, [dict(input=x, block_id=k + 1)])[0]['output'])
    return blocks


def numpy_rag(seg, ignore_label):
    """The restatement the tests use: shifted views per axis, np.unique(axis=0) with counts."""
    nodes = np.unique(seg)
    if ignore_label:
        nodes = nodes[nodes != 0]
    pairs = []
    for axis in range(3):
        lo, hi = [slice(None)] * 3, [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        u, v = seg[tuple(lo)].ravel(), seg[tuple(hi)].ravel()
        keep = u != v
        if ignore_label:
            keep &= (u != 0) & (v != 0)
        u, v = u[keep], v[keep]
        pairs.append(np.stack([np.minimum(u, v), np.maximum(u, v)], axis=1))
    edges, counts = np.unique(np.concatenate(pairs), axis=0, return_counts=True)
    return nodes, edges, counts.astype(np.uint64)


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
    args = ap.parse_args()
    import torch
    from cluster_tools_amd import ctws
    dev = torch.device('cuda', 0)
    h = ctws.Handle(0)
    distinct = make_blocks(h, args.distinct, dev)
    n_vox1 = int(np.prod(SHAPE))
    for nb in (1, args.batch):
        src = [distinct[i % len(distinct)] for i in range(nb)]
        dev_blocks = [torch.from_numpy(lab.view(np.int64)).to(dev) for lab in src]
        n_vox = nb * n_vox1
        rec = {'blocks': nb, 'shape': list(SHAPE)}

        t, res = timed(lambda: [h.rag_block_device(b, True) for b in dev_blocks], args.warmup, args.reps)
        tm = h.timings()
        rec.update(nodes_per_block=[int(len(r[0])) for r in res[:len(distinct)]],
                   edges_per_block=[int(len(r[1])) for r in res[:len(distinct)]],
                   face_pairs_per_voxel=round(float(res[0][2].sum().item()) / n_vox1, 4),
                   device_ms=round(t * 1e3, 3), device_gvox_s=round(n_vox / t / 1e9, 3),
                   stages_ms_last_block={k: round(v, 4) for k, v in tm.items()})
        if 'rag_pairs' in tm:
            rec['pair_stage_stream_tb_s'] = round(n_vox1 * 8 / (tm['rag_pairs'] * 1e-3) / 1e12, 3)
        new_dev = [tuple(a.cpu().numpy().view(np.uint64) for a in r) for r in res]
        if args.device_only:
            print(json.dumps(rec), flush=True)
            continue

        t, res = timed(lambda: [h.rag_block(lab, True) for lab in src], 1, max(1, args.reps // 2))
        rec.update(host_ms=round(t * 1e3, 2), host_gvox_s=round(n_vox / t / 1e9, 3))
        same = all(np.array_equal(a, b) for rd, rh in zip(new_dev, res) for a, b in zip(rd, rh))
        if nb == 1:
            t0 = time.perf_counter()
            ref = numpy_rag(src[0], True)
            t = time.perf_counter() - t0
            rec.update(numpy_one_core_ms=round(t * 1e3, 1), numpy_one_core_gvox_s=round(n_vox1 / t / 1e9, 4))
            same = same and all(np.array_equal(a, b) for a, b in zip(new_dev[0], ref))
        rec['same_result'] = bool(same)
        print(json.dumps(rec), flush=True)
    h.close()


if __name__ == '__main__':
    main()
