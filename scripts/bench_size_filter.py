"""Throughput of the filling size filter (ctws_size_filter_blocks, k_sizefilter.hip + the uint64 /
raw-height-map mode of the from_seeds flood) on one MI355X, next to what the library could do for
the same job before it existed: np.isin on the host plus Handle.ws_from_seeds.

Workload: 64 x 512 x 512 blocks of synthetic DT-watershed fragments (the GPU watershed of the
synthetic boundary map), discard set = the ids below the median size, height map = the
boundary map scaled to min 0 / max 1, so that ws_from_seeds' normalize is the identity and both
paths flood the same values.  One block and a batch of 16, HBM-resident (torch tensors,
ctws_size_filter_blocks_device) and through host pointers (numpy in / out, PCIe included).
Times are host clocks around calls that return after the stream has drained; warm-up calls
first.  The membership kernel's share is the library's own event timing of k_sf_member
(Handle.timings()).  One JSON line per configuration on stdout.
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
    """(labels uint64, hmap float32 in [0, 1]) per distinct block, and the discard ids."""
    from cluster_tools_amd.synthetic import boundary_map_torch
    cfg = dict(size_filter=0, apply_dt_2d=False, apply_ws_2d=False, sigma_seeds=2.0)
    blocks, discard = [], []
    for k in range(n_distinct):
        x = boundary_map_torch(SHAPE, seed=50 + k, device=device).cpu().numpy()
        x = ((x - x.min()) / (x.max() - x.min())).astype(np.float32)
        assert x.min() == 0.0 and x.max() == 1.0
        lab = h.ws_blocks(cfg, SHAPE, [dict(input=x, block_id=k + 1)])[0]['output']
        ids, counts = np.unique(lab, return_counts=True)
        counts, ids = counts[ids != 0], ids[ids != 0]
        discard.append(ids[counts < np.median(counts)])
        blocks.append((lab, x))
    return blocks, np.unique(np.concatenate(discard)).astype(np.uint64)


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
    args = ap.parse_args()
    import torch
    from cluster_tools_amd import ctws
    dev = torch.device('cuda', 0)
    h = ctws.Handle(0)
    distinct, discard = make_blocks(h, args.distinct, dev)
    h.set_discard_ids(discard)
    n_frag = [len(np.unique(lab)) for lab, _ in distinct]
    for nb in (1, args.batch):
        src = [distinct[i % len(distinct)] for i in range(nb)]
        n_vox = nb * int(np.prod(SHAPE))
        host_blocks = [dict(labels=lab, hmap=x, out=np.empty(SHAPE, np.uint64)) for lab, x in src]
        dev_blocks = [dict(labels=torch.from_numpy(lab.view(np.int64)).to(dev), hmap=torch.from_numpy(x).to(dev),
                           out=torch.empty(SHAPE, dtype=torch.int64, device=dev)) for lab, x in src]
        rec = {'blocks': nb, 'shape': list(SHAPE), 'fragments_per_block': n_frag[:nb], 'discard_ids': int(len(discard)),
               'discarded_voxel_share': round(float(np.isin(src[0][0], discard).mean()), 4)}

        t, res = timed(lambda: h.size_filter_blocks_device(dev_blocks, fill=True), args.warmup, args.reps)
        tm = h.timings()
        assert all(r['status'] == ctws.CTWS_BLOCK_WRITTEN for r in res), h.last_error()
        rec.update(device_ms=round(t * 1e3, 2), device_gvox_s=round(n_vox / t / 1e9, 3),
                   member_kernel_ms=round(tm.get('sf_member', float('nan')), 3),
                   member_share=round(tm.get('sf_member', float('nan')) / (t * 1e3), 4))
        new_dev = [r['output'].cpu().numpy().view(np.uint64) for r in res]

        t, res = timed(lambda: h.size_filter_blocks(host_blocks, fill=True), 1, max(1, args.reps // 2))
        rec.update(host_ms=round(t * 1e3, 2), host_gvox_s=round(n_vox / t / 1e9, 3))
        new_host = [r['output'] for r in res]

        # the composition the library offered before: membership on the host, then the seeded flood
        def old():
            seeds = [np.where(np.isin(lab, discard), np.uint64(0), lab) for lab, _ in src]
            return h.ws_from_seeds({'size_filter': 0}, [dict(input=x, seeds=s) for (_, x), s in zip(src, seeds)])
        t, res = timed(old, 1, max(1, args.reps // 2))
        rec.update(isin_from_seeds_ms=round(t * 1e3, 2), isin_from_seeds_gvox_s=round(n_vox / t / 1e9, 3))
        t0 = time.perf_counter()
        np.isin(src[0][0], discard)
        rec['isin_one_block_ms'] = round((time.perf_counter() - t0) * 1e3, 2)
        rec['same_result'] = bool(all(np.array_equal(a, b) and np.array_equal(a, r['output'])
                                      for a, b, r in zip(new_dev, new_host, res)))
        print(json.dumps(rec), flush=True)
    h.close()


if __name__ == '__main__':
    main()
