// k_morph.hip — MorphologyWorkflow on gfx950: size, centre of mass and bounding box of every id
// of a block of uint64 labels.
//
// Reference: morphology/block_morphology.py:111-136 (`ndist.computeAndSerializeMorphology(seg,
// block.begin, ...)`), restated in DESIGN.md section 3.7: for every id of the block (0 included)
// the row [id, n, com_z, com_y, com_x, min_z, min_y, min_x, max_z, max_y, max_x] over its voxels
// at global coordinates begin + local, minima and maxima inclusive, com = float64(sum) / float64(n).
//
//   k_morph_runs  one pass over the block, 8 B per voxel.  A wave owns a (z, y) row and walks it
//                 in words of 64 voxels with coalesced loads.  A lane heads a run when it is the
//                 word's first or its predecessor holds another id (__shfl_up + ballot); the run's
//                 length comes from rag_run_len, so a run never crosses a word and is at most 64
//                 long.  Only heads are emitted, as (id, z:19 | y:19 | x0:19 | len-1:6): 16 B per
//                 run, the two halves in two arrays (the sort's keys and values).  The emits are
//                 staged per wave in LDS and appended with one device-scope atomicAdd per full
//                 stage, as in k_rag_pairs; the counter keeps counting past the capacity and
//                 nothing is written there, so the host re-runs with the counted size.
//                 The same pass takes the largest id (one atomicMax per wave).
//   the sort      sort_pairs_u64 (k_prims.hip) with the ids as keys over the bits of the largest id,
//                 runs_u64 (k_prims.hip) on the sorted ids: the id table and each id's record
//                 count.
//   k_morph_rows  one wave per id: its lanes stride over the id's records and accumulate ten
//                 integers (n, three coordinate sums in uint64, three minima, three maxima), a
//                 fixed butterfly finishes them, the block's begin is added and lanes 0..10 store
//                 the doubles.  Integer sums: the rows do not depend on the append order.  A
//                 segment that holds whole aligned chunks of kMorphChunk records is split: those
//                 chunks go to waves of their own, all parts meet in a per-id table by integer
//                 atomicAdd / atomicMax (still exact), k_morph_long_rows stores those rows.
// Index arithmetic inside a block is 32-bit (a block holds fewer than 2^31 voxels, every extent
// is below 2^19) with one 32-bit division per row, on a wave-uniform value.
#include "ctws_kernels.h"

namespace ctws {

constexpr int kMorphStage = 256;  // staged emits per wave (a step emits at most 64)

__global__ void __launch_bounds__(256) k_morph_runs(MorphArgs a) {
    __shared__ ulonglong2 sr[4][kMorphStage];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t rows = a.nz * a.ny, W = (a.nx + 63u) >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    ulonglong2* __restrict__ sr_w = sr[wv];
    uint32_t fill = 0;  // staged emits of this wave (wave-uniform)
    uint64_t vmax = 0;  // the largest id this lane has seen
    // the wave's staged emits -> the record buffers: one atomicAdd, coalesced stores
    auto flush = [&]() {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.count, (unsigned long long)fill);
        base = (unsigned long long)__shfl((long long)base, 0);
        for (uint32_t k = lane; k < fill; k += 64u) {
            const unsigned long long p = base + k;
            if (p < a.cap) {
                const ulonglong2 rec = sr_w[k];
                a.ids[p] = rec.x;
                a.recs[p] = rec.y;
            }
        }
        __builtin_amdgcn_wave_barrier();
        fill = 0;
    };
    for (uint32_t r = wave0; r < rows; r += nwaves) {
        const uint32_t z = r / a.ny, y = r - z * a.ny;
        const uint32_t rb = r * a.nx;
        const uint64_t zy = ((uint64_t)z << 44) | ((uint64_t)y << 25);
        for (uint32_t w = 0; w < W; ++w) {
            const uint32_t x = (w << 6) + lane;
            const bool in = x < a.nx;
            const uint64_t v = in ? a.lab[rb + x] : 0ull;
            vmax = v > vmax ? v : vmax;
            const uint64_t im = __ballot(in);
            // a lane heads a run when it is the word's first or its predecessor holds another id
            const uint64_t vp = (uint64_t)__shfl_up((long long)v, 1);
            const bool head = in && (lane == 0 || vp != v);
            const uint64_t hm = __ballot(head);
            const uint32_t ne = (uint32_t)__popcll(hm);
            if (fill + ne > (uint32_t)kMorphStage) flush();
            if (head) {
                const uint32_t k = fill + (uint32_t)__popcll(hm & below);
                const uint32_t len = rag_run_len(im & ~hm, lane);
                sr_w[k] = make_ulonglong2(v, zy | ((uint64_t)x << 6) | (uint64_t)(len - 1u));
            }
            __builtin_amdgcn_wave_barrier();
            fill += ne;
        }
    }
    if (fill) flush();
    // the largest id (the sort's bits, the 2^53 limit): one atomicMax per wave, beside its last append
    for (int s = 32; s > 0; s >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((long long)vmax, s);
        vmax = o > vmax ? o : vmax;
    }
    if (lane == 0 && vmax) atomicMax(a.vmax, (unsigned long long)vmax);
}

// first index with sorted[idx] >= v (sorted ascending and holding v)
__device__ __forceinline__ uint32_t morph_first(const uint64_t* __restrict__ sorted, uint32_t n, uint64_t v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct MorphAcc {
    uint64_t n, sz, sy, sx;
    uint32_t lz, ly, lx, hz, hy, hx;
};

__device__ __forceinline__ void morph_add(MorphAcc& c, uint64_t rec) {
    const uint32_t len = (uint32_t)(rec & 63ull) + 1u;
    const uint32_t x0 = (uint32_t)(rec >> 6) & 0x7FFFFu;
    const uint32_t y = (uint32_t)(rec >> 25) & 0x7FFFFu;
    const uint32_t z = (uint32_t)(rec >> 44) & 0x7FFFFu;
    c.n += len;
    c.sx += (uint64_t)(len * x0 + ((len * (len - 1u)) >> 1));  // (64 * 2^19 + 2016 < 2^32)
    c.sy += (uint64_t)(len * y);
    c.sz += (uint64_t)(len * z);
    c.lx = min(c.lx, x0);
    c.hx = max(c.hx, x0 + len - 1u);
    c.ly = min(c.ly, y);
    c.hy = max(c.hy, y);
    c.lz = min(c.lz, z);
    c.hz = max(c.hz, z);
}

// the records [lo, hi) into c: four per lane and step, so that the loads overlap
__device__ __forceinline__ void morph_span(MorphAcc& c, const uint64_t* __restrict__ recs, uint32_t lo, uint32_t hi,
                                           uint32_t lane) {
    uint32_t k = lo + lane;
    for (; k + 192u < hi; k += 256u) {
        const uint64_t r0 = recs[k], r1 = recs[k + 64u], r2 = recs[k + 128u], r3 = recs[k + 192u];
        morph_add(c, r0);
        morph_add(c, r1);
        morph_add(c, r2);
        morph_add(c, r3);
    }
    for (; k < hi; k += 64u) morph_add(c, recs[k]);
}

// the fixed butterfly: every lane ends with the wave's ten integers
__device__ __forceinline__ void morph_reduce(MorphAcc& c) {
    for (int s = 32; s > 0; s >>= 1) {
        c.n += (uint64_t)__shfl_xor((long long)c.n, s);
        c.sz += (uint64_t)__shfl_xor((long long)c.sz, s);
        c.sy += (uint64_t)__shfl_xor((long long)c.sy, s);
        c.sx += (uint64_t)__shfl_xor((long long)c.sx, s);
        c.lz = min(c.lz, (uint32_t)__shfl_xor((int)c.lz, s));
        c.ly = min(c.ly, (uint32_t)__shfl_xor((int)c.ly, s));
        c.lx = min(c.lx, (uint32_t)__shfl_xor((int)c.lx, s));
        c.hz = max(c.hz, (uint32_t)__shfl_xor((int)c.hz, s));
        c.hy = max(c.hy, (uint32_t)__shfl_xor((int)c.hy, s));
        c.hx = max(c.hx, (uint32_t)__shfl_xor((int)c.hx, s));
    }
}

// column `col` of the row of id from its ten integers, in global coordinates: begin + local
// (sums below 2^52: exact in a double)
__device__ __forceinline__ double morph_col(uint32_t col, uint64_t id, uint64_t n, uint64_t sz, uint64_t sy,
                                            uint64_t sx, uint64_t lz, uint64_t ly, uint64_t lx, uint64_t hz,
                                            uint64_t hy, uint64_t hx, const MorphBegin& b) {
    const double dn = (double)n;
    switch (col) {
        case 0: return (double)id;
        case 1: return dn;
        case 2: return (double)(sz + b.z * n) / dn;
        case 3: return (double)(sy + b.y * n) / dn;
        case 4: return (double)(sx + b.x * n) / dn;
        case 5: return (double)(b.z + lz);
        case 6: return (double)(b.y + ly);
        case 7: return (double)(b.x + lx);
        case 8: return (double)(b.z + hz);
        case 9: return (double)(b.y + hy);
        default: return (double)(b.x + hx);
    }
}

// the wave's ten integers into the per-id table: one atomic instruction of ten lanes.  Minima are
// kept as 2^32 - 1 - min, so that a table of zeros is the neutral element of every column
__device__ __forceinline__ void morph_atomics(const MorphAcc& c, unsigned long long* __restrict__ acc, uint32_t lane) {
    switch (lane) {
        case 0: atomicAdd(acc + 0, (unsigned long long)c.n); break;
        case 1: atomicAdd(acc + 1, (unsigned long long)c.sz); break;
        case 2: atomicAdd(acc + 2, (unsigned long long)c.sy); break;
        case 3: atomicAdd(acc + 3, (unsigned long long)c.sx); break;
        case 4: atomicMax(acc + 4, (unsigned long long)(~c.lz)); break;
        case 5: atomicMax(acc + 5, (unsigned long long)(~c.ly)); break;
        case 6: atomicMax(acc + 6, (unsigned long long)(~c.lx)); break;
        case 7: atomicMax(acc + 7, (unsigned long long)c.hz); break;
        case 8: atomicMax(acc + 8, (unsigned long long)c.hy); break;
        case 9: atomicMax(acc + 9, (unsigned long long)c.hx); break;
        default: break;
    }
}

// Waves [0, m): one per id.  An id whose segment of the sorted records holds no whole aligned chunk
// of kMorphChunk records (fewer than 2 chunks: nearly every fragment) is finished here and its row
// stored.  A longer segment (a background id can own half of a block's records) gives this wave
// only its head and tail, up to the chunk borders; the aligned chunks in between go to the waves
// [m, m + n / kMorphChunk), one chunk each, which find a chunk of one id by its first and last
// key.  Both kinds add their ten integers into the id's line of acc (zeroed; integer atomics: exact
// and independent of the order); k_morph_long_rows stores those rows.
__global__ void __launch_bounds__(256) k_morph_rows(const uint64_t* __restrict__ sorted_ids,
                                                    const uint64_t* __restrict__ sorted_recs, uint32_t n,
                                                    const uint64_t* __restrict__ uniq,
                                                    const uint64_t* __restrict__ counts, uint32_t m, MorphBegin b,
                                                    unsigned long long* __restrict__ acc, double* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    constexpr uint32_t K = (uint32_t)kMorphChunk;
    const uint32_t chunks = n / K;
    for (uint32_t w = wave0; w < m + chunks; w += nwaves) {
        MorphAcc c = {0ull, 0ull, 0ull, 0ull, ~0u, ~0u, ~0u, 0u, 0u, 0u};
        if (w < m) {
            const uint64_t id = uniq[w];
            const uint32_t cnt = (uint32_t)counts[w];
            const uint32_t first = morph_first(sorted_ids, n, id);
            // (first + cnt <= n by construction; the clamp keeps a corrupted table inside the buffer)
            const uint32_t end = min(first + cnt, n);
            const uint32_t hs = ((first + K - 1u) / K) * K, te = (end / K) * K;  // the aligned chunks: [hs, te)
            if (hs >= te) {
                morph_span(c, sorted_recs, first, end, lane);
                morph_reduce(c);
                if (lane < 11u)
                    out[(size_t)w * 11u + lane] =
                        morph_col(lane, id, c.n, c.sz, c.sy, c.sx, c.lz, c.ly, c.lx, c.hz, c.hy, c.hx, b);
            } else {
                morph_span(c, sorted_recs, first, hs, lane);
                morph_span(c, sorted_recs, te, end, lane);
                morph_reduce(c);
                if (c.n) morph_atomics(c, acc + (size_t)w * 10u, lane);
            }
        } else {
            const uint32_t lo = (w - m) * K;  // (lo + K <= n)
            const uint64_t id = sorted_ids[lo];
            if (id != sorted_ids[lo + K - 1u]) continue;  // an id border inside: the ids' own waves take it
            uint32_t i = 0, hi = m;  // the id's line: first index with uniq[i] >= id
            while (i < hi) {
                const uint32_t mid = i + ((hi - i) >> 1);
                if (uniq[mid] < id) i = mid + 1;
                else hi = mid;
            }
            if (i >= m) continue;
            morph_span(c, sorted_recs, lo, lo + K, lane);
            morph_reduce(c);
            morph_atomics(c, acc + (size_t)i * 10u, lane);
        }
    }
}

// the rows of the ids that k_morph_rows accumulated in acc (n != 0 there)
__global__ void __launch_bounds__(256) k_morph_long_rows(const uint64_t* __restrict__ uniq, uint32_t m, MorphBegin b,
                                                         const unsigned long long* __restrict__ acc,
                                                         double* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const unsigned long long* __restrict__ a = acc + (size_t)i * 10u;
        if (a[0] == 0ull) continue;
        const uint64_t id = uniq[i];
        for (uint32_t col = 0; col < 11u; ++col)
            out[(size_t)i * 11u + col] =
                morph_col(col, id, a[0], a[1], a[2], a[3], (uint64_t)(~(uint32_t)a[4]), (uint64_t)(~(uint32_t)a[5]),
                          (uint64_t)(~(uint32_t)a[6]), a[7], a[8], a[9], b);
    }
}

}  // namespace ctws
