// k_regfeat.hip — RegionFeaturesWorkflow on gfx950: the number of voxels and the mean input value
// of every id of a block of uint64 labels.
//
// Reference: features/region_features.py:119-160 (`vigra.analysis.extractRegionFeatures(input,
// labels, features=['mean', 'count'], ignoreLabel=...)` on `vu.normalize(input)`), restated in
// a voxel's value is float32 (uint8 / 255, every other dtype cast), an id's
// row is [id, n, float64(sum of its values) / float64(n)], the ignore label's row is [id, 0, 0].
//
// Float sums do not commute, so nothing here depends on the order in which waves run: no
// floating-point atomic, no atomic append.  Every record has a place that follows from the labels.
//
//   k_regfeat_count  labels only, 8 B per voxel.  A wave owns a (z, y) row, walks it in words of 64
//                    voxels and writes the row's number of run heads (a head: the word's first
//                    lane, or a lane whose predecessor holds another id).  An exclusive scan over
//                    the rows (k_prims.hip) gives each row's first record and the total, which sizes the
//                    record arrays exactly.
//   k_regfeat_runs   labels and values, coalesced.  The run sums come from a segmented inclusive
//                    scan over the word in float64: six shuffle steps, a lane adds only what lies
//                    at or after its run's head, so a run's sum is a function of the word.  A head
//                    stores its record at (row's first record + heads before it in the row): the id
//                    (the sort's key), (run length << 32 | record index) (the sort's value) and the
//                    float64 sum at the record index.  Runs of the ignore label get length 0 and
//                    sum 0.  The same pass takes the largest id (one integer atomicMax per wave).
//   the sort         sort_pairs_u64 (k_prims.hip; the LSD radix sort is stable, so an id's records
//                    stay in scan order) over the bits of the largest id, runs_u64 on the sorted
//                    ids: the id table and each id's record count.
//   k_regfeat_chunks a wave per whole aligned chunk of kRegfeatChunk sorted records that holds one
//                    id only: its (n, sum) into the chunk table.
//   k_regfeat_rows   a wave per id.  Lane l takes the records first + l, first + l + 64, ... of the
//                    id's head (up to the first chunk border), then its chunks' table entries in
//                    ascending index, then its tail; n in uint64, the sum in float64, a fixed
//                    butterfly finishes both and lanes 0..2 store [id, n, n ? sum / n : 0].  What a
//                    lane adds, and in which order, follows from the sorted positions alone.
// Index arithmetic inside a block is 32-bit (a block holds fewer than 2^31 voxels).
#include "ctws_kernels.h"

namespace ctws {

// a lane heads a run when it is the word's first or its predecessor holds another id
__device__ __forceinline__ uint64_t regfeat_heads(uint64_t v, bool in, uint32_t lane) {
    const uint64_t vp = (uint64_t)__shfl_up((long long)v, 1);
    return __ballot(in && (lane == 0 || vp != v));
}

__global__ void __launch_bounds__(256) k_regfeat_count(const uint64_t* __restrict__ lab, uint32_t rows, uint32_t nx,
                                                       uint32_t* __restrict__ row_heads) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t W = (nx + 63u) >> 6;
    for (uint32_t r = wave0; r < rows; r += nwaves) {
        const uint32_t rb = r * nx;
        uint32_t heads = 0;
        for (uint32_t w = 0; w < W; ++w) {
            const uint32_t x = (w << 6) + lane;
            const bool in = x < nx;
            const uint64_t v = in ? lab[rb + x] : 0ull;
            heads += (uint32_t)__popcll(regfeat_heads(v, in, lane));
        }
        if (lane == 0) row_heads[r] = heads;
    }
}

// the value of a voxel: vu.normalize(x, 0, 255 if uint8 else 1) in float32
__device__ __forceinline__ float regfeat_value(uint8_t v) { return (float)v / 255.0f; }
__device__ __forceinline__ float regfeat_value(uint16_t v) { return (float)v; }
__device__ __forceinline__ float regfeat_value(float v) { return v; }
__device__ __forceinline__ float regfeat_value(double v) { return (float)v; }  // (round to nearest)

template <class T>
__global__ void __launch_bounds__(256) k_regfeat_runs(RegfeatArgs a) {
    const T* __restrict__ data = (const T*)a.data;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t W = (a.nx + 63u) >> 6;
    const uint64_t upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;  // the lanes 0..lane
    const uint64_t below = (1ull << lane) - 1ull;
    uint64_t vmax = 0;  // the largest id this lane has seen
    for (uint32_t r = wave0; r < a.rows; r += nwaves) {
        const uint32_t rb = r * a.nx;
        uint32_t base = a.row_first[r];  // the row's first record (wave-uniform)
        for (uint32_t w = 0; w < W; ++w) {
            const uint32_t x = (w << 6) + lane;
            const bool in = x < a.nx;
            const uint64_t v = in ? a.lab[rb + x] : 0ull;
            const bool ign = a.with_ignore && v == a.ignore;
            double s = (in && !ign) ? (double)regfeat_value(data[rb + x]) : 0.0;
            vmax = v > vmax ? v : vmax;
            const uint64_t im = __ballot(in);
            const uint64_t hm = regfeat_heads(v, in, lane);
            // the lane of this lane's run head: the last head at or below it (lanes past the row's
            // end head no run: they take the row's last head and add 0 to their own s, which
            // nothing reads; lane 0 only when the word holds no head at all)
            const uint64_t hb = hm & upto;
            const uint32_t hl = hb ? 63u - (uint32_t)__builtin_clzll(hb) : 0u;
            // segmented inclusive scan: after step d a lane holds the sum of the up to 2d lanes
            // ending at it that lie in its run
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const double o = __shfl_up(s, d);
                if (lane >= hl + d) s += o;
            }
            const bool head = (hm >> lane) & 1ull;
            const uint32_t len = head ? rag_run_len(im & ~hm, lane) : 1u;
            const double rs = __shfl(s, (int)(lane + len - 1u));  // the run's last lane holds its sum
            if (head) {
                const uint32_t p = base + (uint32_t)__popcll(hm & below);
                if (p < a.n) {  // (always: the count pass saw the same labels)
                    a.ids[p] = v;
                    a.vals[p] = ((uint64_t)(ign ? 0u : len) << 32) | (uint64_t)p;
                    a.sums[p] = rs;
                }
            }
            base += (uint32_t)__popcll(hm);
        }
    }
    for (int s = 32; s > 0; s >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((long long)vmax, s);
        vmax = o > vmax ? o : vmax;
    }
    if (lane == 0 && vmax) atomicMax(a.vmax, (unsigned long long)vmax);
}

template __global__ void k_regfeat_runs<uint8_t>(RegfeatArgs);
template __global__ void k_regfeat_runs<uint16_t>(RegfeatArgs);
template __global__ void k_regfeat_runs<float>(RegfeatArgs);
template __global__ void k_regfeat_runs<double>(RegfeatArgs);

// first index with sorted[idx] >= v (sorted ascending and holding v)
__device__ __forceinline__ uint32_t regfeat_first(const uint64_t* __restrict__ sorted, uint32_t n, uint64_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the sum of record v, by its index in the low word ((always) below nrec: the clamp keeps a
// corrupted value inside the buffer)
__device__ __forceinline__ double regfeat_sum(const double* __restrict__ sums, uint32_t nrec, uint64_t v) {
    return sums[min((uint32_t)v, nrec - 1u)];
}

// the sorted records [lo, hi) into this lane's (n, s): lane l takes lo + l, lo + l + 64, ...
__device__ __forceinline__ void regfeat_span(uint64_t& n, double& s, const uint64_t* __restrict__ svals,
                                             const double* __restrict__ sums, uint32_t nrec, uint32_t lo, uint32_t hi,
                                             uint32_t lane) {
    uint32_t k = lo + lane;
    // four per lane and step, so that the gathers overlap; the adds keep their order
    for (; k + 192u < hi; k += 256u) {
        const uint64_t v0 = svals[k], v1 = svals[k + 64u], v2 = svals[k + 128u], v3 = svals[k + 192u];
        const double s0 = regfeat_sum(sums, nrec, v0), s1 = regfeat_sum(sums, nrec, v1);
        const double s2 = regfeat_sum(sums, nrec, v2), s3 = regfeat_sum(sums, nrec, v3);
        n += (v0 >> 32) + (v1 >> 32) + (v2 >> 32) + (v3 >> 32);
        s += s0;
        s += s1;
        s += s2;
        s += s3;
    }
    for (; k < hi; k += 64u) {
        const uint64_t v = svals[k];
        n += v >> 32;
        s += regfeat_sum(sums, nrec, v);
    }
}

// the fixed butterfly: every lane ends with the wave's n and sum (a + b == b + a, so all lanes agree)
__device__ __forceinline__ void regfeat_reduce(uint64_t& n, double& s) {
    for (int d = 32; d > 0; d >>= 1) {
        n += (uint64_t)__shfl_xor((long long)n, d);
        s += __shfl_xor(s, d);
    }
}

__global__ void __launch_bounds__(256) k_regfeat_chunks(const uint64_t* __restrict__ sorted_ids,
                                                        const uint64_t* __restrict__ svals,
                                                        const double* __restrict__ sums, uint32_t n,
                                                        uint64_t* __restrict__ chunk_n, double* __restrict__ chunk_s) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    constexpr uint32_t K = (uint32_t)kRegfeatChunk;
    const uint32_t chunks = n / K;
    for (uint32_t c = wave0; c < chunks; c += nwaves) {
        const uint32_t lo = c * K;  // (lo + K <= n)
        if (sorted_ids[lo] != sorted_ids[lo + K - 1u]) continue;  // an id border inside: the ids' own waves take it
        uint64_t cn = 0;
        double cs = 0.0;
        regfeat_span(cn, cs, svals, sums, n, lo, lo + K, lane);
        regfeat_reduce(cn, cs);
        if (lane == 0) {
            chunk_n[c] = cn;
            chunk_s[c] = cs;
        }
    }
}

__global__ void __launch_bounds__(256) k_regfeat_rows(const uint64_t* __restrict__ sorted_ids,
                                                      const uint64_t* __restrict__ svals,
                                                      const double* __restrict__ sums, uint32_t n,
                                                      const uint64_t* __restrict__ uniq,
                                                      const uint64_t* __restrict__ counts, uint32_t m,
                                                      const uint64_t* __restrict__ chunk_n,
                                                      const double* __restrict__ chunk_s, double* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    constexpr uint32_t K = (uint32_t)kRegfeatChunk;
    for (uint32_t w = wave0; w < m; w += nwaves) {
        const uint64_t id = uniq[w];
        const uint32_t cnt = (uint32_t)counts[w];
        const uint32_t first = regfeat_first(sorted_ids, n, id);
        // (first + cnt <= n by construction; the clamp keeps a corrupted table inside the buffer)
        const uint32_t end = min(first + cnt, n);
        const uint32_t hs = ((first + K - 1u) / K) * K, te = (end / K) * K;  // the aligned chunks: [hs, te)
        uint64_t rn = 0;
        double rs = 0.0;
        if (hs >= te) {
            regfeat_span(rn, rs, svals, sums, n, first, end, lane);
        } else {
            regfeat_span(rn, rs, svals, sums, n, first, hs, lane);
            for (uint32_t c = hs / K + lane; c < te / K; c += 64u) {
                rn += chunk_n[c];
                rs += chunk_s[c];
            }
            regfeat_span(rn, rs, svals, sums, n, te, end, lane);
        }
        regfeat_reduce(rn, rs);
        if (lane < 3u) {
            const double dn = (double)rn;
            out[(size_t)w * 3u + lane] = lane == 0 ? (double)id : lane == 1 ? dn : (rn ? rs / dn : 0.0);
        }
    }
}

}  // namespace ctws
