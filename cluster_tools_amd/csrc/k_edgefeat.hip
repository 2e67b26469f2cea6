// k_edgefeat.hip — EdgeFeaturesWorkflow on gfx950: the boundary-map statistics of a block's edges.
//
// Reference: features/block_edge_features.py:113-132 (`ndist.extractBlockFeaturesFromBoundaryMaps_*`
// per block, increaseRoi=True).  nifty is not available: the semantics are restated in DESIGN.md
// section 3.5.  Per edge of the block's sub-graph, over the face-adjacent voxel pairs (p, p + e)
// with p in the core box, p + e in the extended box and different (not ignored) ids: both voxel
// values are samples of the edge; the row is [mean, variance, min, q10, q25, q50, q75, q90, max,
// count] with exact order statistics.
//
//   k_ef_edge_keys  edge (u, v) -> rank(u) << b | rank(v) in the block's node table (the ranking of
//                   k_pair_keys).  The edges are sorted, so the keys ascend: an edge whose
//                   endpoint is no node, or a key that does not exceed its predecessor, is counted.
//   k_ef_samples    one pass over the core rows, 8 B of labels + 1 or 4 B of data per voxel, with
//                   the traversal of k_rag_pairs: a wave owns a row and walks it in words of 64
//                   voxels, the +x neighbour comes from the next lane, +y / +z from coalesced loads
//                   of the two adjacent rows, and one ballot skips a word inside a fragment before
//                   any data is read.  No run compression (the values differ along a run).  A
//                   lane finds its own rank once, the ranks of its +y / +z neighbours by a search
//                   each and the rank of the +x neighbour in the next lane; the edge index is a
//                   search in the key table.  Every owned pair emits two 64-bit keys
//                   edge << 32 | ordered(value), staged per wave in LDS and appended with one
//                   atomicAdd per full stage; past the capacity the counter keeps counting and
//                   nothing is written (the protocol of k_rag_pairs).
//   sort_keys_u64   radix sort of the keys over the bits [0, 32 + bits(n_edges)) (k_prims.hip): the
//                   samples of an edge become one ascending segment.  The append order does not
//                   matter: equal keys are equal samples.
//   k_ef_stats      one wave per edge: the segment by two searches, per-lane double partial sums
//                   in index order and a fixed butterfly (the result depends on the sorted data
//                   alone), a second sweep for the variance, the quantiles by direct indexing.
// Index arithmetic inside a block is 32-bit.  No float atomics anywhere: the results are
// bit-reproducible.
#include "ctws_kernels.h"

#pragma clang fp contract(off)

namespace ctws {

// first index with tab[idx] >= v, 32-bit
__device__ __forceinline__ uint32_t ef_lower(const uint64_t* __restrict__ tab, uint32_t nt, uint64_t v) {
    uint32_t lo = 0, hi = nt;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid] < v) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// rank of v in tab, or 0xffffffff when v is not in it
__device__ __forceinline__ uint32_t ef_rank(const uint64_t* __restrict__ tab, uint32_t nt, uint64_t v) {
    const uint32_t r = ef_lower(tab, nt, v);
    return (r < nt && tab[r] == v) ? r : 0xffffffffu;
}

constexpr uint32_t kEfNone = 0xffffffffu;

__device__ __forceinline__ uint64_t ef_edge_key(const uint64_t* __restrict__ edges, int64_t i,
                                                const uint64_t* __restrict__ tab, uint32_t nt, int b, bool& ok) {
    const ulonglong2 e = ((const ulonglong2*)edges)[i];
    const uint32_t ru = ef_rank(tab, nt, e.x), rv = ef_rank(tab, nt, e.y);
    ok = ru != kEfNone && rv != kEfNone;
    return ((uint64_t)ru << b) | (uint64_t)rv;
}

__global__ void __launch_bounds__(256) k_ef_edge_keys(const uint64_t* __restrict__ edges, int64_t n,
                                                      const uint64_t* __restrict__ tab, int64_t nt, int b,
                                                      uint64_t* __restrict__ keys, unsigned long long* __restrict__ bad) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        bool ok, okp = true;
        const uint64_t k = ef_edge_key(edges, i, tab, (uint32_t)nt, b, ok);
        const uint64_t kp = i ? ef_edge_key(edges, i - 1, tab, (uint32_t)nt, b, okp) : 0ull;
        if (!ok || (i && okp && kp >= k)) atomicAdd(bad, 1ull);
        keys[i] = k;
    }
}

// the monotone map float32 -> uint32 (all bits flipped under the sign, else the sign bit set)
__device__ __forceinline__ uint32_t ef_ordered(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ef_unordered(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

template <class T>
__device__ __forceinline__ float ef_value(const T* __restrict__ d, uint32_t i);
template <>
__device__ __forceinline__ float ef_value<float>(const float* __restrict__ d, uint32_t i) {
    return d[i];
}
template <>
__device__ __forceinline__ float ef_value<uint8_t>(const uint8_t* __restrict__ d, uint32_t i) {
    return (float)d[i] / 255.0f;
}

constexpr int kEfStage = 1024;  // staged keys per wave (a step emits at most 3 * 64 * 2)

template <class T>
__global__ void __launch_bounds__(256) k_ef_samples(EfArgs a) {
    __shared__ uint64_t sk[4][kEfStage];
    const T* __restrict__ data = (const T*)a.data;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    // only rows and words with a voxel of the core box own a pair
    const uint32_t rows = a.cz * a.cy, W = (a.cx + 63u) >> 6;
    const uint32_t sy = a.nx, sz = a.ny * a.nx;
    const uint64_t below = (1ull << lane) - 1ull;
    uint64_t* __restrict__ sk_w = sk[wv];
    uint32_t fill = 0;  // staged keys of this wave (wave-uniform)
    unsigned long long miss = 0;  // this lane's pairs without an edge
    auto flush = [&]() {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.count, (unsigned long long)fill);
        base = (unsigned long long)__shfl((long long)base, 0);
        for (uint32_t k = lane; k < fill; k += 64u) {
            const unsigned long long p = base + k;
            if (p < a.cap) a.keys[p] = sk_w[k];
        }
        __builtin_amdgcn_wave_barrier();
        fill = 0;
    };
    // the index of the edge between ranks r0 and r1 (different), or kEfNone
    auto edge_of = [&](uint32_t r0, uint32_t r1) -> uint32_t {
        if (r0 == kEfNone || r1 == kEfNone) return kEfNone;
        const uint64_t k = r0 < r1 ? ((uint64_t)r0 << a.b) | r1 : ((uint64_t)r1 << a.b) | r0;
        const uint32_t e = ef_lower(a.ekeys, a.ne, k);
        return (e < a.ne && a.ekeys[e] == k) ? e : kEfNone;
    };
    for (uint32_t r = wave0; r < rows; r += nwaves) {
        const uint32_t z = r / a.cy, y = r - z * a.cy;
        const bool hy = y + 1u < a.ny, hz = z + 1u < a.nz;
        const uint32_t rb = (z * a.ny + y) * a.nx;
        for (uint32_t w = 0; w < W; ++w) {
            const uint32_t x = (w << 6) + lane;
            const bool in = x < a.nx, own = x < a.cx, hx = x + 1u < a.nx;
            const uint32_t i = rb + x;
            const uint64_t v = in ? a.lab[i] : 0ull;
            const uint64_t vy = own && hy ? a.lab[i + sy] : 0ull;
            const uint64_t vz = own && hz ? a.lab[i + sz] : 0ull;
            const uint64_t vn = (uint64_t)__shfl_down((long long)v, 1);
            const uint64_t vx = lane == 63 && hx ? a.lab[i + 1u] : vn;
            const bool nz0 = !a.ignore || v != 0ull;
            const bool dx = own && hx && v != vx && nz0 && (!a.ignore || vx != 0ull);
            const bool dy = own && hy && v != vy && nz0 && (!a.ignore || vy != 0ull);
            const bool dz = own && hz && v != vz && nz0 && (!a.ignore || vz != 0ull);
            const uint64_t mx = __ballot(dx), my = __ballot(dy), mz = __ballot(dz);
            if ((mx | my | mz) == 0ull) continue;  // a fragment's interior: no data is read
            // the values: the lane's own (also the +x neighbour of its predecessor), +y, +z
            const float f = in ? ef_value<T>(data, i) : 0.f;
            const float fn = __shfl_down(f, 1);
            const float fx = lane == 63 && dx ? ef_value<T>(data, i + 1u) : fn;
            const float fy = dy ? ef_value<T>(data, i + sy) : 0.f;
            const float fz = dz ? ef_value<T>(data, i + sz) : 0.f;
            // ranks: the lane's own once (wanted by itself or by its predecessor's x pair)
            const bool want = dx || dy || dz || (lane > 0 && ((mx >> (lane - 1u)) & 1ull));
            const uint32_t ru = want ? ef_rank(a.tab, a.nt, v) : kEfNone;
            const uint32_t rn = (uint32_t)__shfl_down((int)ru, 1);
            const uint32_t rx = dx ? (lane == 63 ? ef_rank(a.tab, a.nt, vx) : rn) : kEfNone;
            const uint32_t ex_ = dx ? edge_of(ru, rx) : kEfNone;
            const uint32_t ey_ = dy ? edge_of(ru, ef_rank(a.tab, a.nt, vy)) : kEfNone;
            const uint32_t ez_ = dz ? edge_of(ru, ef_rank(a.tab, a.nt, vz)) : kEfNone;
            miss += (dx && ex_ == kEfNone) + (dy && ey_ == kEfNone) + (dz && ez_ == kEfNone);
            const bool px = ex_ != kEfNone, py = ey_ != kEfNone, pz = ez_ != kEfNone;
            const uint64_t bx = __ballot(px), by = __ballot(py), bz = __ballot(pz);
            const uint32_t nxe = 2u * (uint32_t)__popcll(bx), nye = 2u * (uint32_t)__popcll(by),
                           nze = 2u * (uint32_t)__popcll(bz);
            if (nxe + nye + nze == 0u) continue;
            if (fill + nxe + nye + nze > (uint32_t)kEfStage) flush();  // (a step emits at most 384)
            const uint32_t of = ef_ordered(f);
            if (px) {
                const uint32_t k = fill + 2u * (uint32_t)__popcll(bx & below);
                sk_w[k] = ((uint64_t)ex_ << 32) | of;
                sk_w[k + 1u] = ((uint64_t)ex_ << 32) | ef_ordered(fx);
            }
            if (py) {
                const uint32_t k = fill + nxe + 2u * (uint32_t)__popcll(by & below);
                sk_w[k] = ((uint64_t)ey_ << 32) | of;
                sk_w[k + 1u] = ((uint64_t)ey_ << 32) | ef_ordered(fy);
            }
            if (pz) {
                const uint32_t k = fill + nxe + nye + 2u * (uint32_t)__popcll(bz & below);
                sk_w[k] = ((uint64_t)ez_ << 32) | of;
                sk_w[k + 1u] = ((uint64_t)ez_ << 32) | ef_ordered(fz);
            }
            __builtin_amdgcn_wave_barrier();
            fill += nxe + nye + nze;
        }
    }
    if (fill) flush();
    if (miss) atomicAdd(a.missing, miss);
}
template __global__ void k_ef_samples<float>(EfArgs);
template __global__ void k_ef_samples<uint8_t>(EfArgs);

// a fixed butterfly: every lane ends with the same sum, whatever the hardware does elsewhere
__device__ __forceinline__ double ef_wave_sum(double s) {
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
    return s;
}

__global__ void __launch_bounds__(256) k_ef_stats(const uint64_t* __restrict__ keys, uint32_t n, uint32_t ne,
                                                  double* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (e >= ne) return;
    const uint32_t s0 = ef_lower(keys, n, (uint64_t)e << 32);
    const uint32_t s1 = ef_lower(keys, n, ((uint64_t)e + 1ull) << 32);
    const uint32_t m = s1 - s0;  // samples = 2 * pairs
    double val = 0.0;
    if (m) {
        const uint64_t* __restrict__ seg = keys + s0;
        auto at = [&](uint32_t i) -> double { return (double)ef_unordered((uint32_t)seg[i]); };
        double s = 0.0;
        for (uint32_t i = lane; i < m; i += 64u) s = s + at(i);
        const double mean = ef_wave_sum(s) / (double)m;
        double q = 0.0;
        for (uint32_t i = lane; i < m; i += 64u) {
            const double d = at(i) - mean;
            q = q + d * d;
        }
        const double var = ef_wave_sum(q) / (double)m;
        // lanes 2 .. 8: min (q = 0), the five quantiles, max (q = 1) by the same formula
        const double qs = lane == 2 ? 0.0 : lane == 3 ? 0.1 : lane == 4 ? 0.25 : lane == 5 ? 0.5
                        : lane == 6 ? 0.75 : lane == 7 ? 0.9 : 1.0;
        const double pos = qs * (double)(m - 1u);
        const uint32_t l = (uint32_t)pos;  // (pos >= 0: the truncation is the floor)
        const uint32_t hgh = l + 1u < m ? l + 1u : m - 1u;
        const double sl = at(l), sh = at(hgh);
        const double qv = sl + (pos - (double)l) * (sh - sl);
        val = lane == 0 ? mean : lane == 1 ? var : lane == 9 ? (double)(m >> 1) : qv;
    }
    if (lane < 10u) out[(size_t)e * 10u + lane] = val;
}

}  // namespace ctws
