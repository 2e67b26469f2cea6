"""Throughput of the morphology table of a block (ctws_block_morphology, k_morph.hip) on one
MI355X, next to ctws_rag_block on the same blocks in the same run and the numpy restatement
(tests/morphology_ref.py) on one CPU core.

Workload: 64 x 512 x 512 blocks of synthetic DT-watershed fragments, one block and 16 (the entry
point takes one block: 16 calls), HBM-resident (torch tensors, ctws_block_morphology_device; the
rows stay in HBM) and through host pointers (numpy in / out, PCIe included).  Times are host
clocks around calls that return after the stream has drained; warm-up calls first.  The stage
split is the library's own event timing of the last device call (Handle.timings(); a stage's span
includes its host round trips -- kernel times proper come from a kernel trace of this script,
--device-only).  The run kernel's rate is given as bytes of an 8 B per voxel stream over its span.
--background F zeroes a fraction F of every block's fragments first (one id that owns many
records: the long segment of k_morph_rows).  One JSON line per configuration on stdout.
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


def make_blocks(h, n_distinct, device, background):
    from cluster_tools_amd.synthetic import boundary_map_torch
    cfg = dict(size_filter=25, apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=2.0)
    blocks = []
    for k in range(n_distinct):
        x = np.ascontiguousarray(boundary_map_torch(SHAPE, seed=50 + k, device=device).cpu().numpy(), dtype=np.float32)
        lab = h.ws_blocks(cfg, SHAPE, [dict(input=x, block_id=k + 1)])[0]['output']
        if background > 0:
            ids = np.unique(lab)
            drop = ids[np.random.RandomState(k).rand(len(ids)) < background]
            lab = np.where(np.isin(lab, drop), np.uint64(0), lab)
        blocks.append(np.ascontiguousarray(lab, dtype=np.uint64))
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
    ap.add_argument('--background', type=float, default=0., help='fraction of the fragments set to 0')
    ap.add_argument('--device-only', action='store_true', help='HBM-resident calls only (for a kernel trace)')
    ap.add_argument('--no-numpy', action='store_true', help='skip the restatement on one core')
    args = ap.parse_args()
    import torch
    from cluster_tools_amd import ctws
    dev = torch.device('cuda', 0)
    h = ctws.Handle(0)
    distinct = make_blocks(h, args.distinct, dev, args.background)
    begin = (128, 1024, 512)
    n_vox1 = int(np.prod(SHAPE))
    for nb in (1, args.batch):
        src = [distinct[i % len(distinct)] for i in range(nb)]
        dev_lab = [torch.from_numpy(lab.view(np.int64)).to(dev) for lab in src]
        n_vox = nb * n_vox1
        rec = {'blocks': nb, 'shape': list(SHAPE), 'background': args.background}

        t, _ = timed(lambda: [h.rag_block_device(b, True) for b in dev_lab], args.warmup, args.reps)
        rec.update(rag_device_ms=round(t * 1e3, 3), rag_device_gvox_s=round(n_vox / t / 1e9, 3),
                   rag_stages_ms_last_block={k: round(v, 4) for k, v in h.timings().items()})

        t, res = timed(lambda: [h.block_morphology_device(b, begin) for b in dev_lab], args.warmup, args.reps)
        tm = h.timings()
        new_dev = [r.cpu().numpy() for r in res]
        rec.update(ids_per_block=[int(len(r)) for r in new_dev[:len(distinct)]],
                   largest_size_fraction=round(float(new_dev[0][:, 1].max()) / n_vox1, 4),
                   device_ms=round(t * 1e3, 3), device_gvox_s=round(n_vox / t / 1e9, 3),
                   stages_ms_last_block={k: round(v, 4) for k, v in tm.items()})
        if 'morph_emits' in tm:
            rec['records_per_voxel'] = round(tm['morph_emits'] / n_vox1, 4)
        if 'morph_runs' in tm:
            rec['run_stage_stream_tb_s'] = round(n_vox1 * 8 / (tm['morph_runs'] * 1e-3) / 1e12, 3)
        if args.device_only:
            print(json.dumps(rec), flush=True)
            continue

        t, _ = timed(lambda: [h.rag_block(lab, True) for lab in src], 1, max(1, args.reps // 2))
        rec.update(rag_host_ms=round(t * 1e3, 2), rag_host_gvox_s=round(n_vox / t / 1e9, 3))
        t, res = timed(lambda: [h.block_morphology(lab, begin) for lab in src], 1, max(1, args.reps // 2))
        rec.update(host_ms=round(t * 1e3, 2), host_gvox_s=round(n_vox / t / 1e9, 3))
        rec['same_result'] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(new_dev, res)))
        if nb == 1 and not args.no_numpy:
            import morphology_ref as M
            t0 = time.perf_counter()
            ref = M.block_morphology(src[0], begin)
            t = time.perf_counter() - t0
            rec.update(numpy_one_core_ms=round(t * 1e3, 1), numpy_one_core_gvox_s=round(n_vox1 / t / 1e9, 4))
            rec['equals_numpy'] = bool(np.array_equal(new_dev[0], ref))
        print(json.dumps(rec), flush=True)
    h.close()


if __name__ == '__main__':
    main()
