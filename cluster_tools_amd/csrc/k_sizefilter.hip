// k_sizefilter.hip — the global size filter's block kernels on gfx950.
//
// Reference: postprocess/background_size_filter.py:110-130 and filling_size_filter.py:112-136
// (`apply_block`): discard_mask = np.in1d(labels, discard_ids); labels[discard_mask] = 0; the
// filling variant then floods the raw height map from the labels that are left
// (vigra watershedsNew, 3-D direct nbhd).
//
//   k_sf_member  one pass over a block's uint64 labels: seeds = labels with 0 where the id is in
//                the discard set, and three per-block facts in BlockStat (active: a nonzero
//                label; fg: discarded voxels; _p[2..3]: the largest id kept).  Labels come in
//                runs along x, so a wave looks an id up once per run: a lane is a run head if it
//                is lane 0 or its label differs from its predecessor's in the flat index (rows
//                do not start on wave boundaries), the heads look up (one bitmap word, or a
//                binary search of the sorted table), and every lane takes the answer of the
//                nearest head at or below it with one shuffle.  The facts are reduced with
//                ballots and a wave max: at most three atomics per wave, none per voxel.
//   k_sf_hmap    the filling flood's height map: the raw input cast to float32 (exact for u8,
//                u16 and f32) -- no normalize, clamp, invert or mask (vu.normalize is affine in
//                float32 and can merge distinct values, which changes ties).
#include "ctws_kernels.h"

namespace ctws {

__device__ __forceinline__ bool sf_lookup(const SfDiscard& d, uint64_t v) {
    if (v < d.lo || v > d.hi) return false;  // (an empty set has lo > hi)
    if (d.bits) {
        const uint64_t o = v - d.lo;
        return (gbl(d.bits)[o >> 6] >> (o & 63)) & 1ull;
    }
    int64_t lo = 0, hi = d.n;  // first index with ids[idx] >= v
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (gbl(d.ids)[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo < d.n && gbl(d.ids)[lo] == v;
}

__global__ void __launch_bounds__(256) k_sf_member(const SfBlock* __restrict__ D, BlockStat* S, SfDiscard d) {
    const SfBlock B = D[blockIdx.y];
    const int lane = threadIdx.x & 63;
    // lanes at or below this one (the nearest run head is the highest head bit among them)
    const uint64_t at_or_below = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
    uint32_t any = 0, ndisc = 0;
    uint64_t mx = 0;
    // (four pieces per iteration with their label loads in flight together measured the same:
    // 2.55 -> 2.64 ms for 16 blocks of 64 x 512 x 512)
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63); i0 < B.N;
         i0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = i0 + lane;
        const bool in = i < B.N;
        const uint64_t v = in ? gbl(B.lab)[i] : 0ull;
        const uint64_t prev = (uint64_t)__shfl_up((long long)v, 1);
        const bool head = lane == 0 || v != prev;
        const uint64_t heads = __ballot(head);
        int disc = 0;
        if (head && in) disc = sf_lookup(d, v) ? 1 : 0;
        disc = __shfl(disc, 63 - __clzll((long long)(heads & at_or_below)));
        const uint64_t keep = disc ? 0ull : v;
        if (in) B.seeds[i] = keep;
        any |= __ballot(v != 0ull) != 0ull ? 1u : 0u;
        ndisc += (uint32_t)__popcll(__ballot(in && disc));
        mx = keep > mx ? keep : mx;
    }
    for (int s = 32; s > 0; s >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((long long)mx, s);
        mx = o > mx ? o : mx;
    }
    if (lane == 0) {
        BlockStat& st = S[blockIdx.y];
        if (any) atomicOr(&st.active, 1u);
        if (ndisc) atomicAdd(&st.fg, ndisc);
        if (mx) atomicMax((unsigned long long*)&st._p[2], (unsigned long long)mx);
    }
}

template <class T>
__device__ __forceinline__ void sf_cast(const BlockDesc& B, float* __restrict__ hm) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < B.N; i += (int64_t)gridDim.x * blockDim.x)
        hm[B.base + i] = (float)gbl((const T*)B.input)[i];
}

__global__ void __launch_bounds__(256) k_sf_hmap(const BlockDesc* __restrict__ D, float* __restrict__ hm) {
    const BlockDesc& B = D[blockIdx.y];
    if (B.dtype == 1) sf_cast<uint8_t>(B, hm);        // CTWS_U8
    else if (B.dtype == 2) sf_cast<uint16_t>(B, hm);  // CTWS_U16
    else sf_cast<float>(B, hm);                       // CTWS_F32 (other dtypes are refused on the host)
}

}  // namespace ctws
