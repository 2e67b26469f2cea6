"""Throughput of the image filter of a block (ctws_image_filter, k_imgfilter.hip) on one MI355X,
next to the numpy restatement (tests/image_filter_ref.py) and scipy.ndimage.gaussian_filter on one
CPU core, for scale.

Workload: 64 x 512 x 512 float32 blocks of uniform noise, one block and 16 (the entry point takes
one block: 16 calls), sigma 1.6 (radii 5 and 6) and 4.0 (radii 12, 14, 16), the three filters,
normalize on; HBM-resident (torch tensors, ctws_image_filter_device) and through host pointers
(numpy in / out, PCIe included).  Times are host clocks around calls that return after the stream
has drained; warm-up calls first.  The pass split is the library's own event timing of the last
device call (Handle.timings()); kernel times proper come from a kernel trace of this script,
--device-only.  Each pass's rate is its in + out bytes per voxel (derived from the shapes: minmax
4; smoothing 4 + 4 per pass; derivative filters 4 + 8, 8 + 12, 12 + 4) over its span.  A
single-output composition of a derivative filter is nine passes like the smoothing call's three
plus a combine: three smoothing calls of the same run are its lower bound (the derivative taps are
longer), printed as composed_lower_bound_ms.  A streaming kernel of the same run for scale: the
(2, 2, 2) float32 mean of ctws_downscale_block_device (4.5 B per input voxel).  One JSON line per
configuration on stdout; profiles/image_filter/bench_image_filter.jsonl is that output of a full
run, kernel_stats.csv beside it the statistics of a kernel trace of `--device-only --batch 1`.
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
FILTERS = ('gaussianSmoothing', 'gaussianGradientMagnitude', 'laplacianOfGaussian')
PASS_BYTES = {False: {'if_minmax': 4, 'if_first': 8, 'if_y': 8, 'if_x': 8},
              True: {'if_minmax': 4, 'if_first': 12, 'if_y': 20, 'if_x': 16}}


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
    ap.add_argument('--sigmas', type=float, nargs='+', default=[1.6, 4.0])
    ap.add_argument('--shape', type=int, nargs=3, default=list(SHAPE))
    ap.add_argument('--device-only', action='store_true', help='HBM-resident calls only (for a kernel trace)')
    ap.add_argument('--no-cpu', action='store_true', help='skip the restatement and scipy on one core')
    args = ap.parse_args()
    import torch
    from cluster_tools_amd import ctws
    shape = tuple(args.shape)
    dev = torch.device('cuda', 0)
    h = ctws.Handle(0)
    rng = np.random.RandomState(7)
    distinct = [rng.rand(*shape).astype('float32') for _ in range(2)]
    n_vox1 = int(np.prod(shape))
    for nb in (1, args.batch):
        src = [distinct[i % 2] for i in range(nb)]
        dev_src = [torch.from_numpy(x).to(dev) for x in distinct]
        dev_src = [dev_src[i % 2] for i in range(nb)]
        n_vox = nb * n_vox1
        t, _ = timed(lambda: [h.downscale_block_device(x, (2, 2, 2), 'mean') for x in dev_src], args.warmup, args.reps)
        ds_kernel_ms = h.timings().get('downscale')
        for sigma in args.sigmas:
            smooth_ms = None
            for name in FILTERS:
                rec = {'blocks': nb, 'shape': list(shape), 'filter': name, 'sigma': sigma,
                       'downscale_222_stage_ms': round(ds_kernel_ms, 4),
                       'downscale_222_tb_s': round(n_vox1 * 4.5 / (ds_kernel_ms * 1e-3) / 1e12, 3)}
                t, res = timed(lambda: [h.image_filter_device(x, name, sigma) for x in dev_src],
                               args.warmup, args.reps)
                tm = h.timings()
                per_voxel = PASS_BYTES[name != 'gaussianSmoothing']
                rec.update(device_ms=round(t * 1e3, 3), device_gvox_s=round(n_vox / t / 1e9, 3),
                           device_in_out_tb_s=round(n_vox * sum(per_voxel.values()) / t / 1e12, 3),
                           passes_ms_last_block={k: round(v, 4) for k, v in tm.items()},
                           passes_tb_s_last_block={k: round(n_vox1 * per_voxel[k] / (v * 1e-3) / 1e12, 3)
                                                   for k, v in tm.items() if v > 0})
                if name == 'gaussianSmoothing':
                    smooth_ms = t * 1e3
                else:
                    rec['composed_lower_bound_ms'] = round(3 * smooth_ms, 3)
                first_dev = res[0].cpu().numpy()
                if not args.device_only:
                    t, res = timed(lambda: [h.image_filter(x, name, sigma) for x in src], args.warmup, args.reps)
                    rec.update(host_ms=round(t * 1e3, 2), host_gvox_s=round(n_vox / t / 1e9, 3),
                               same_result=bool(np.array_equal(res[0], first_dev)))
                    if nb == 1 and sigma == args.sigmas[0] and not args.no_cpu:
                        import image_filter_ref as R
                        from scipy import ndimage
                        t0 = time.perf_counter()
                        ref = R.apply_filter(src[0], name, sigma, taps_fn=ctws.filter_taps)
                        t = time.perf_counter() - t0
                        rec.update(numpy_one_core_ms=round(t * 1e3, 1),
                                   numpy_one_core_gvox_s=round(n_vox1 / t / 1e9, 4),
                                   equals_numpy=bool(np.array_equal(first_dev, ref)))
                        order = R.ORDER[name]
                        t0 = time.perf_counter()
                        if order == 0:
                            ndimage.gaussian_filter(src[0], sigma, mode='mirror')
                        else:  # three components, as the filters need them
                            for d in range(3):
                                ndimage.gaussian_filter(src[0], sigma, order=[order if a == d else 0 for a in range(3)],
                                                        mode='mirror')
                        t = time.perf_counter() - t0
                        rec.update(scipy_one_core_ms=round(t * 1e3, 1), scipy_one_core_gvox_s=round(n_vox1 / t / 1e9, 4))
                print(json.dumps(rec), flush=True)
    h.close()


if __name__ == '__main__':
    main()
