"""Throughput of the fragment / label overlaps of a block (ctws_label_overlaps, k_overlaps.hip) on
one MI355X, next to ctws_rag_block on the same fragments in the same run and the numpy
restatement (tests/node_labels_ref.py) on one CPU core.

Workload: 64 x 512 x 512 blocks of synthetic DT-watershed fragments; the label volume of a block
is the fragment volume of another seed (a second segmentation of the same size and coherence), one
block and 16 (the entry point takes one block: 16 calls), HBM-resident (torch tensors,
ctws_label_overlaps_device; the rows stay in HBM) and through host pointers (numpy in / out, PCIe
included).  Times are host clocks around calls that return after the stream has drained; warm-up
calls first.  The stage split is the library's own event timing of the last device call
(Handle.timings(); a stage's span includes its host round trips -- kernel times proper come from a
kernel trace of this script, --device-only).  The pair kernel's rate is given as bytes of its
16 B per voxel stream over its span.  One JSON line per configuration on stdout.
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
        blocks.append(h.ws_blocks(cfg, SHAPE, [dict(input=x, block_id=k + 1)])[0]['output'])
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
    ap.add_argument('--ignore-label', type=int, default=0, help='-1: no ignore label')
    ap.add_argument('--device-only', action='store_true', help='HBM-resident calls only (for a kernel trace)')
    ap.add_argument('--no-numpy', action='store_true', help='skip the restatement on one core')
    args = ap.parse_args()
    assert args.distinct >= 2, "the label volume of a block is another block's fragments"
    ignore_label = None if args.ignore_label < 0 else args.ignore_label
    import torch
    from cluster_tools_amd import ctws
    dev = torch.device('cuda', 0)
    h = ctws.Handle(0)
    distinct = make_blocks(h, args.distinct, dev)
    n_vox1 = int(np.prod(SHAPE))
    for nb in (1, args.batch):
        src = [(distinct[i % len(distinct)], distinct[(i + 1) % len(distinct)]) for i in range(nb)]
        dev_src = [tuple(torch.from_numpy(a.view(np.int64)).to(dev) for a in pair) for pair in src]
        n_vox = nb * n_vox1
        rec = {'blocks': nb, 'shape': list(SHAPE), 'ignore_label': ignore_label}

        t, _ = timed(lambda: [h.rag_block_device(n, True) for n, _ in dev_src], args.warmup, args.reps)
        rec.update(rag_device_ms=round(t * 1e3, 3), rag_device_gvox_s=round(n_vox / t / 1e9, 3))

        t, res = timed(lambda: [h.label_overlaps_device(n, l, ignore_label) for n, l in dev_src],
                       args.warmup, args.reps)
        tm = h.timings()
        rec.update(rows_per_block=[int(len(r)) for r in res[:len(distinct)]],
                   device_ms=round(t * 1e3, 3), device_gvox_s=round(n_vox / t / 1e9, 3),
                   stages_ms_last_block={k: round(v, 4) for k, v in tm.items()})
        if 'ov_pairs' in tm:
            rec['pair_stage_stream_tb_s'] = round(n_vox1 * 16 / (tm['ov_pairs'] * 1e-3) / 1e12, 3)
        rec['device_over_rag'] = round(rec['device_gvox_s'] / rec['rag_device_gvox_s'], 3)
        new_dev = [r.cpu().numpy().view(np.uint64) for r in res]
        if args.device_only:
            print(json.dumps(rec), flush=True)
            continue

        t, _ = timed(lambda: [h.rag_block(n, True) for n, _ in src], 1, max(1, args.reps // 2))
        rec.update(rag_host_ms=round(t * 1e3, 2), rag_host_gvox_s=round(n_vox / t / 1e9, 3))
        t, res = timed(lambda: [h.label_overlaps(n, l, ignore_label) for n, l in src], 1, max(1, args.reps // 2))
        rec.update(host_ms=round(t * 1e3, 2), host_gvox_s=round(n_vox / t / 1e9, 3))
        rec['same_result'] = bool(all(np.array_equal(a, b) for a, b in zip(new_dev, res)))
        if nb == 1 and not args.no_numpy:
            import node_labels_ref as R
            t0 = time.perf_counter()
            ref = R.overlap_rows(src[0][0], src[0][1], ignore_label)
            t = time.perf_counter() - t0
            rec.update(numpy_one_core_ms=round(t * 1e3, 1), numpy_one_core_gvox_s=round(n_vox1 / t / 1e9, 4))
            rec['equal_to_numpy'] = bool(np.array_equal(new_dev[0], ref))
        print(json.dumps(rec), flush=True)
    h.close()


if __name__ == '__main__':
    main()
