"""Throughput of one block of the scale pyramid (ctws_downscale_block, k_downscale.hip) on one
MI355X, next to ctws_block_morphology on blocks of the same shape in the same run (this
repository's own 8 B per voxel stream) and the numpy restatement (tests/downscaling_ref.py) on one
CPU core.

Workload: 64 x 512 x 512 blocks of random uint8 and float32 voxels, factors (1, 2, 2) and
(2, 2, 2), mean; one block, and a batch of distinct blocks that does not fit the 256 MiB Infinity
Cache (16 float32 blocks are 1 GiB, 32 uint8 blocks 512 MiB; the entry point takes one block, so a
batch is that many calls).  HBM-resident (torch tensors, ctws_downscale_block_device; the output
stays in HBM) and through host pointers (numpy in / out, PCIe included).  Times are host clocks
around calls that return after the stream has drained, warm-up calls first; a call on a block this
small is mostly its launch and its round trip for the flag, so the kernel's own span (the
library's event timing, memset of the flag included; the median over the batch's calls) is given
next to it with the bytes it moves, in + out.  One JSON line per configuration on stdout.
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
BATCH = {'uint8': 32, 'float32': 16}


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def make_blocks(torch, dev, dtype, n):
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    if dtype == 'uint8':
        return [torch.randint(0, 256, SHAPE, dtype=torch.uint8, device=dev, generator=g) for _ in range(n)]
    return [torch.randn(SHAPE, dtype=torch.float32, device=dev, generator=g) for _ in range(n)]


def morphology_yardstick(h, torch, dev, warmup, reps):
    """block_morphology on two watershed label blocks of the same shape: the call rate and the
    run pass's rate as an 8 B per voxel stream."""
    from cluster_tools_amd.synthetic import boundary_map_torch
    cfg = dict(size_filter=25, apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=2.0)
    labs = []
    for k in range(2):
        x = np.ascontiguousarray(boundary_map_torch(SHAPE, seed=50 + k, device=dev).cpu().numpy(), dtype=np.float32)
        lab = h.ws_blocks(cfg, SHAPE, [dict(input=x, block_id=k + 1)])[0]['output']
        labs.append(torch.from_numpy(np.ascontiguousarray(lab, dtype=np.uint64).view(np.int64)).to(dev))
    n_vox1 = int(np.prod(SHAPE))
    src = [labs[i % 2] for i in range(16)]
    t, _ = timed(lambda: [h.block_morphology_device(b, (0, 0, 0)) for b in src], warmup, reps)
    runs = []
    for b in src:
        h.block_morphology_device(b, (0, 0, 0))
        runs.append(h.timings()['morph_runs'])
    run_ms = float(np.median(runs))
    return {'yardstick': 'block_morphology', 'blocks': 16, 'shape': list(SHAPE),
            'device_ms': round(t * 1e3, 3), 'device_gvox_s': round(16 * n_vox1 / t / 1e9, 3),
            'run_pass_ms': round(run_ms, 4), 'run_pass_gb_s': round(n_vox1 * 8 / (run_ms * 1e-3) / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--device-only', action='store_true', help='HBM-resident calls only (for a kernel trace)')
    ap.add_argument('--no-numpy', action='store_true', help='skip the restatement on one core')
    ap.add_argument('--no-yardstick', action='store_true', help='skip block_morphology')
    args = ap.parse_args()
    import torch
    from cluster_tools_amd import ctws
    import downscaling_ref as R
    dev = torch.device('cuda', 0)
    h = ctws.Handle(0)
    n_vox1 = int(np.prod(SHAPE))
    if not args.no_yardstick:
        print(json.dumps(morphology_yardstick(h, torch, dev, args.warmup, args.reps)), flush=True)
    for dtype in ('uint8', 'float32'):
        distinct = make_blocks(torch, dev, dtype, BATCH[dtype])
        es = distinct[0].element_size()
        host = None if args.device_only else [b.cpu().numpy() for b in distinct]
        for factors in ((1, 2, 2), (2, 2, 2)):
            n_out1 = int(np.prod([-(-s // f) for s, f in zip(SHAPE, factors)]))
            bytes1 = (n_vox1 + n_out1) * es
            for nb in (1, BATCH[dtype]):
                src = distinct[:nb]
                n_vox = nb * n_vox1
                rec = {'dtype': dtype, 'factors': list(factors), 'func': 'mean', 'blocks': nb, 'shape': list(SHAPE),
                       'distinct_input_mib': round(nb * n_vox1 * es / 2 ** 20), 'bytes_per_voxel': bytes1 / n_vox1}
                t, res = timed(lambda: [h.downscale_block_device(b, factors) for b in src], args.warmup, args.reps)
                spans = []
                for b in src:
                    h.downscale_block_device(b, factors)
                    spans.append(h.timings()['downscale'])
                span = float(np.median(spans))
                rec.update(device_ms=round(t * 1e3, 3), device_gvox_s=round(n_vox / t / 1e9, 2),
                           device_gb_s=round(nb * bytes1 / t / 1e9, 1), kernel_span_ms=round(span, 4),
                           kernel_gvox_s=round(n_vox1 / (span * 1e-3) / 1e9, 1),
                           kernel_gb_s=round(bytes1 / (span * 1e-3) / 1e9, 1))
                if not args.device_only:
                    hsrc = host[:nb]
                    t, hres = timed(lambda: [h.downscale_block(x, factors) for x in hsrc], 1, max(1, args.reps // 2))
                    rec.update(host_ms=round(t * 1e3, 2), host_gvox_s=round(n_vox / t / 1e9, 3),
                               host_gb_s=round(nb * bytes1 / t / 1e9, 2))
                    rec['same_result'] = bool(all(a[0].cpu().numpy().tobytes() == b[0].tobytes() and a[1] == b[1]
                                                  for a, b in zip(res, hres)))
                    if nb == 1 and not args.no_numpy:
                        t0 = time.perf_counter()
                        ref = R.reduce_block(hsrc[0], factors)
                        t = time.perf_counter() - t0
                        rec.update(numpy_one_core_ms=round(t * 1e3, 1),
                                   numpy_one_core_gvox_s=round(n_vox1 / t / 1e9, 4))
                        if dtype == 'uint8':
                            rec['equals_numpy'] = bool(np.array_equal(hres[0][0], ref))
                        else:
                            rec['max_abs_diff_numpy'] = float(np.abs(hres[0][0] - ref).max())
                print(json.dumps(rec), flush=True)
        del distinct, host
        torch.cuda.empty_cache()
    h.close()


if __name__ == '__main__':
    main()
