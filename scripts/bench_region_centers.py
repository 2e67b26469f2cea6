"""Throughput of the region centres (ctws_region_centers, k_regcenter.hip) on one MI355X, next to
the reference's per-object `distance_transform_edt` + `np.argmax` on one CPU core on the same boxes
in the same run (scipy if it imports, else the numpy restatement tests/region_centers_ref.py on
the first --baseline-objects boxes; the record says which).

Workload: the synthetic DT-watershed fragments of one 64 x 512 x 512 block.  The boxes come from
`Handle.block_morphology` and follow the task's rule, [min, max) of the table's inclusive extremes
(empty boxes are dropped).  Three forms of the same call: HBM-resident (a torch tensor and the
boxes inside it, ctws_region_centers_device; only the centres come back), host pointers with the
boxes inside the block (the whole block is staged), and host pointers with packed crops (what the
task does; the packing is timed).  Times are host clocks around calls that return after the stream
has drained; warm-up calls first.  The split between the two kernel paths and the library's own
event timing of the last HBM-resident call are recorded.  One JSON line per resolution, appended to
--out (default profiles/region_centers/bench_region_centers.jsonl)."""
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


def make_block(h, device, seed=50):
    from cluster_tools_amd.synthetic import boundary_map_torch
    cfg = dict(size_filter=25, apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=2.0)
    x = np.ascontiguousarray(boundary_map_torch(SHAPE, seed=seed, device=device).cpu().numpy(), dtype=np.float32)
    lab = h.ws_blocks(cfg, SHAPE, [dict(input=x, block_id=1)])[0]['output']
    return np.ascontiguousarray(lab, dtype=np.uint64)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def baseline(lab, ids, boxes, resolution, n_objects):
    """-> (name, seconds, objects, box voxels, centres) on one core."""
    try:
        from scipy.ndimage import distance_transform_edt
        name = 'scipy'
    except ImportError:
        import region_centers_ref as R
        name = 'numpy restatement'
        ids, boxes = ids[:n_objects], boxes[:n_objects]
    centers = np.zeros((len(ids), 3), dtype=np.int64)
    t0 = time.perf_counter()
    for k, (i, b) in enumerate(zip(ids, boxes)):
        obj = lab[b[0]:b[3], b[1]:b[4], b[2]:b[5]] == i
        if name == 'scipy':
            if obj.sum() == 0:
                continue
            centers[k] = np.unravel_index(int(np.argmax(distance_transform_edt(obj, sampling=resolution))), obj.shape)
        else:
            c = R.box_center(obj, resolution)
            if c is not None:
                centers[k] = c
    t = time.perf_counter() - t0
    return name, t, len(ids), int(np.prod(boxes[:, 3:] - boxes[:, :3], axis=1).sum()), centers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--baseline-objects', type=int, default=200, help='boxes of the numpy baseline (scipy: all)')
    ap.add_argument('--no-baseline', action='store_true')
    ap.add_argument('--device-only', action='store_true', help='HBM-resident calls only (for a kernel trace)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'region_centers', 'bench_region_centers.jsonl'))
    args = ap.parse_args()
    import torch
    from cluster_tools_amd import ctws
    dev = torch.device('cuda', 0)
    h = ctws.Handle(0)
    lab = make_block(h, dev)
    rows = h.block_morphology(lab)
    lo, hi = rows[:, 5:8].astype(np.int64), rows[:, 8:11].astype(np.int64)
    keep = (hi > lo).all(axis=1)
    ids = rows[keep, 0].astype(np.uint64)
    boxes = np.concatenate([lo[keep], hi[keep]], axis=1)
    vox = np.prod(boxes[:, 3:] - boxes[:, :3], axis=1)
    n_obj, n_vox = len(ids), int(vox.sum())
    dlab = torch.from_numpy(lab.view(np.int64)).to(dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for resolution in ((1, 1, 1), (10, 1, 1)):
        rec = {'shape': list(SHAPE), 'resolution': list(resolution), 'ids_in_block': int(len(rows)),
               'objects': n_obj, 'box_voxels': n_vox, 'block_voxels': int(lab.size),
               'median_box_voxels': int(np.median(vox)), 'largest_box_voxels': int(vox.max())}
        t, res = timed(lambda: h.region_centers_boxes_device(dlab, ids, boxes, resolution), args.warmup, args.reps)
        tm = h.timings()
        dev_c, dev_f = res[0].cpu().numpy(), res[1].cpu().numpy()
        n_small, n_large = int(tm['rc_small_objects']), int(tm['rc_large_objects'])
        small_vox = int(vox[vox <= h.REGION_CENTERS_SMALL_VOXELS].sum())
        rec.update(device_ms=round(t * 1e3, 3), device_objects_s=round(n_obj / t), device_box_gvox_s=round(n_vox / t / 1e9, 3),
                   small_objects=n_small, large_objects=n_large, small_box_voxels=small_vox,
                   large_box_voxels=n_vox - small_vox, found=int(dev_f.sum()),
                   stages_ms_last_call={k: round(v, 4) for k, v in tm.items()})
        if tm.get('rc_small'):
            rec['small_path_objects_s'] = round(n_small / (tm['rc_small'] * 1e-3))
            rec['small_path_us_per_object'] = round(tm['rc_small'] * 1e3 / max(1, n_small), 3)
        if tm.get('rc_large'):
            rec['large_path_box_gvox_s'] = round((n_vox - small_vox) / (tm['rc_large'] * 1e-3) / 1e9, 3)
        if not args.device_only:
            t, res = timed(lambda: h.region_centers_boxes(lab, ids, boxes, resolution), 1, max(1, args.reps // 2))
            rec.update(host_boxes_ms=round(t * 1e3, 2), host_boxes_objects_s=round(n_obj / t))
            same = res[0].tobytes() == dev_c.tobytes() and res[1].tobytes() == dev_f.tobytes()

            def packed():
                crops = [lab[b[0]:b[3], b[1]:b[4], b[2]:b[5]] for b in boxes]
                return h.region_centers(crops, ids, resolution)
            t, res = timed(packed, 1, max(1, args.reps // 2))
            rec.update(host_crops_ms=round(t * 1e3, 2), host_crops_objects_s=round(n_obj / t),
                       host_crops_box_gvox_s=round(n_vox / t / 1e9, 3))
            rec['same_result'] = bool(same and res[0].tobytes() == dev_c.tobytes() and res[1].tobytes() == dev_f.tobytes())
        if not args.no_baseline and not args.device_only:
            name, t, n, v, ref = baseline(lab, ids, boxes, resolution, args.baseline_objects)
            rec.update(baseline=name, baseline_objects=n, baseline_one_core_ms=round(t * 1e3, 1),
                       baseline_objects_s=round(n / t, 1), baseline_box_gvox_s=round(v / t / 1e9, 4),
                       equals_baseline=bool(np.array_equal(ref, dev_c[:n])),
                       speedup_device_vs_one_core=round((t / n) / (rec['device_ms'] * 1e-3 / n_obj), 1))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')
    h.close()


if __name__ == '__main__':
    main()
