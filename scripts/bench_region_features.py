"""Throughput of the region features of a block (ctws_region_features_block, k_regfeat.hip) on one
MI355X, next to ctws_block_morphology and ctws_label_overlaps on the same blocks in the same run
and a vectorised numpy restatement (unique + bincount) on one CPU core.

Workload: 64 x 512 x 512 blocks of synthetic DT-watershed fragments with the boundary map they were
made from as the input map (float32, and uint8 as round(255 x)), one block and 16 (the entry point
takes one block: 16 calls), HBM-resident (torch tensors, ctws_region_features_block_device; the
rows stay in HBM) and through host pointers (numpy in / out, PCIe included).  Times are host clocks
around calls that return after the stream has drained; warm-up calls first.  The stage split is the
library's own event timing of the last device call (Handle.timings(); a stage's span includes its
host round trips).  The call streams the labels twice and the values once: 20 B per voxel for
float32, 17 for uint8, against morphology's 8 and label_overlaps' 16.
--background F zeroes a fraction F of every block's fragments first and runs with
ignore_label=None (one id that owns many records: the long segment of k_regfeat_rows); without it
ignore_label is 0.  One JSON line per configuration on stdout.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
        blocks.append((np.ascontiguousarray(lab, dtype=np.uint64), x))
    return blocks


def numpy_rows(labels, data, ignore_label):
    """[id, count, mean] per id with numpy on one core: unique + bincount (sums in voxel order)."""
    vals = (data.astype('float32') / np.float32(255.) if data.dtype == np.uint8 else data.astype('float32'))
    ids, inv = np.unique(labels, return_inverse=True)
    inv = inv.ravel()
    count = np.bincount(inv, minlength=len(ids)).astype('float64')
    total = np.bincount(inv, weights=vals.ravel().astype('float64'), minlength=len(ids))
    rows = np.zeros((len(ids), 3))
    rows[:, 0] = ids
    rows[:, 1] = count
    rows[:, 2] = total / count
    if ignore_label is not None:
        rows[ids == ignore_label, 1:] = 0
    return rows


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
    ignore_label = None if args.background > 0 else 0
    n_vox1 = int(np.prod(SHAPE))
    for dtype in ('float32', 'uint8'):
        for nb in (1, args.batch):
            src = [distinct[i % len(distinct)] for i in range(nb)]
            labs = [lab for lab, _ in src]
            maps = [x if dtype == 'float32' else np.round(x * 255).astype('uint8') for _, x in src]
            dev_lab = [torch.from_numpy(lab.view(np.int64)).to(dev) for lab in labs]
            dev_map = [torch.from_numpy(x).to(dev) for x in maps]
            # the second label volume of label_overlaps: the next distinct block's fragments
            dev_other = [dev_lab[(i + 1) % len(distinct)] if nb > 1 else
                         torch.from_numpy(distinct[1 % len(distinct)][0].view(np.int64)).to(dev) for i in range(nb)]
            n_vox = nb * n_vox1
            rec = {'blocks': nb, 'shape': list(SHAPE), 'dtype': dtype, 'background': args.background,
                   'ignore_label': ignore_label}

            t, _ = timed(lambda: [h.block_morphology_device(b) for b in dev_lab], args.warmup, args.reps)
            rec.update(morphology_device_ms=round(t * 1e3, 3), morphology_device_gvox_s=round(n_vox / t / 1e9, 3))
            t, _ = timed(lambda: [h.label_overlaps_device(a, b) for a, b in zip(dev_lab, dev_other)],
                         args.warmup, args.reps)
            rec.update(overlaps_device_ms=round(t * 1e3, 3), overlaps_device_gvox_s=round(n_vox / t / 1e9, 3))

            t, res = timed(lambda: [h.region_features_block_device(a, b, ignore_label)
                                    for a, b in zip(dev_lab, dev_map)], args.warmup, args.reps)
            tm = h.timings()
            new_dev = [r.cpu().numpy() for r in res]
            rec.update(ids_per_block=[int(len(r)) for r in new_dev[:len(distinct)]],
                       largest_count_fraction=round(float(new_dev[0][:, 1].max()) / n_vox1, 4),
                       device_ms=round(t * 1e3, 3), device_gvox_s=round(n_vox / t / 1e9, 3),
                       stages_ms_last_block={k: round(v, 4) for k, v in tm.items() if k != 'regfeat_records'})
            if 'regfeat_records' in tm:
                rec['records_per_voxel'] = round(tm['regfeat_records'] / n_vox1, 4)
            es = 4 if dtype == 'float32' else 1
            if 'regfeat_count' in tm:
                rec['count_stage_stream_tb_s'] = round(n_vox1 * 8 / (tm['regfeat_count'] * 1e-3) / 1e12, 3)
            if 'regfeat_runs' in tm:
                rec['run_stage_stream_tb_s'] = round(n_vox1 * (8 + es) / (tm['regfeat_runs'] * 1e-3) / 1e12, 3)
            if args.device_only:
                print(json.dumps(rec), flush=True)
                continue

            t, _ = timed(lambda: [h.block_morphology(lab) for lab in labs], 1, max(1, args.reps // 2))
            rec.update(morphology_host_ms=round(t * 1e3, 2), morphology_host_gvox_s=round(n_vox / t / 1e9, 3))
            t, res = timed(lambda: [h.region_features_block(a, b, ignore_label) for a, b in zip(labs, maps)],
                           1, max(1, args.reps // 2))
            rec.update(host_ms=round(t * 1e3, 2), host_gvox_s=round(n_vox / t / 1e9, 3))
            rec['same_result'] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(new_dev, res)))
            if nb == 1 and not args.no_numpy:
                t0 = time.perf_counter()
                ref = numpy_rows(labs[0], maps[0], ignore_label)
                t = time.perf_counter() - t0
                rec.update(numpy_one_core_ms=round(t * 1e3, 1), numpy_one_core_gvox_s=round(n_vox1 / t / 1e9, 4))
                got = new_dev[0]
                rec['ids_and_counts_equal_numpy'] = bool(np.array_equal(got[:, :2], ref[:, :2]))
                # (numpy adds in voxel order: the means differ by float64 rounding)
                rec['largest_mean_difference_to_numpy'] = float(np.abs(got[:, 2] - ref[:, 2]).max())
            print(json.dumps(rec), flush=True)
    h.close()


if __name__ == '__main__':
    main()
