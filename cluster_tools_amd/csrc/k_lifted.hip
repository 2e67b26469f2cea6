// k_lifted.hip — LiftedFeaturesFromNodeLabelsWorkflow on gfx950: the sparse lifted neighbourhood of
// a region adjacency graph under a node labelling.
//
// Reference: lifted_features/sparse_lifted_neighborhood.py:131-135
// (`ndist.computeLiftedNeighborhoodFromNodeLabels`; restated in DESIGN.md section 3.12, nifty is not
// available).  The lifted edges are the pairs (u, v), u < v, of labelled nodes at hop distance
// 2 .. depth in the whole graph that pass the mode test on their two labels.
//
//   k_lf_degrees   one pass over the edge table (m x 2): checks every row (ids below n, u < v,
//                  rows strictly ascending) and counts both endpoints' degrees.
//   k_lf_fill      the second pass: adj[row[u] + k] = v and adj[row[v] + k] = u, k from an atomic
//                  cursor per node (the order inside a list does not matter).
//   k_lf_sources   the ids of the labelled nodes, compacted with one atomicAdd per wave.
//   k_lf_bfs       one wave per source, level-synchronous, at most `depth` levels.  The wave keeps
//                  ONE list of the nodes it has reached, in the order it reached them: the first
//                  kLfQueueLds entries in its slice of the LDS, the rest in its slice of a global
//                  queue.  A level is a contiguous range of that list, and the list is also what
//                  clears the bitmap below.  The visited set is an open-addressing hash set in the
//                  wave's LDS (kLfHashSlots words, linear probing of at most kLfProbe slots,
//                  insertion by an LDS compare-and-swap: of two lanes with one node exactly one
//                  sees it as new, so the SET does not depend on which lane wins).  When a probe
//                  runs out or the set holds kLfHashFill nodes, the wave marks every node of its
//                  list in its own global bitmap over the n nodes and goes on there (atomicOr),
//                  and at the end of the source it clears the bitmap by walking the list again,
//                  never by a memset of n bits.  A step takes 64 nodes of the frontier, scans
//                  their degrees across the wave and gives every lane one adjacency entry at a
//                  time (the owner of entry e by a binary search in the scanned degrees in LDS):
//                  a list of 200 entries is spread over the lanes like 64 lists of 3.  A node
//                  first reached at level >= 2 with an id above the source's, a label and a
//                  passing mode test is staged in LDS as source << b | node; a full stage is
//                  appended with ONE atomicAdd (the protocol of k_rag_pairs: the counter keeps
//                  counting past the capacity and nothing is written there).  Every loop is
//                  bounded by the depth, the probe limit, a list's length or the node count.
//   sort_keys_u64 (k_prims.hip) / k_lf_unpack  radix sort of the keys over their 2 b bits, key -> (u, v) rows.
// Integer arithmetic only; node ids and adjacency offsets are 32-bit (n < 2^32, 2 m < 2^32), the
// emit counter is 64-bit.
#include "ctws_kernels.h"

namespace ctws {

__global__ void __launch_bounds__(256) k_lf_degrees(const uint64_t* __restrict__ edges, uint32_t m, uint64_t n,
                                                    uint32_t* __restrict__ deg, unsigned long long* __restrict__ bad) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const ulonglong2 e = ((const ulonglong2*)edges)[i];
        const bool in = e.x < n && e.y < n;
        if (!in) atomicAdd(bad + kLfBadId, 1ull);
        if (e.x >= e.y) atomicAdd(bad + kLfBadUv, 1ull);
        if (i > 0u) {
            const ulonglong2 p = ((const ulonglong2*)edges)[i - 1u];
            if (!(p.x < e.x || (p.x == e.x && p.y < e.y))) atomicAdd(bad + kLfBadOrder, 1ull);
        }
        if (in) {
            atomicAdd(deg + (uint32_t)e.x, 1u);
            atomicAdd(deg + (uint32_t)e.y, 1u);
        }
    }
}

// (the rows passed k_lf_degrees: every id is below n; cur is zeroed)
__global__ void __launch_bounds__(256) k_lf_fill(const uint64_t* __restrict__ edges, uint32_t m,
                                                 const uint32_t* __restrict__ row, uint32_t* __restrict__ cur,
                                                 uint32_t* __restrict__ adj) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const ulonglong2 e = ((const ulonglong2*)edges)[i];
        const uint32_t u = (uint32_t)e.x, v = (uint32_t)e.y;
        adj[row[u] + atomicAdd(cur + u, 1u)] = v;
        adj[row[v] + atomicAdd(cur + v, 1u)] = u;
    }
}

__global__ void __launch_bounds__(256) k_lf_sources(const uint64_t* __restrict__ lab, uint32_t n, uint64_t ignore,
                                                    uint32_t* __restrict__ src, unsigned long long* __restrict__ count) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n64 = (n + 63u) & ~63u;  // (whole waves take the loop together; n + 63 < 2^32)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n64; i += gridDim.x * blockDim.x) {
        const bool s = i < n && lab[i] != ignore;
        const uint64_t ms = __ballot(s);
        if (ms == 0ull) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(count, (unsigned long long)__popcll(ms));
        base = (unsigned long long)__shfl((long long)base, 0);
        if (s) src[base + (uint32_t)__popcll(ms & ((1ull << lane) - 1ull))] = i;
    }
}

// what one lane wrote, LDS or global, is read by another lane of the wave behind this
__device__ __forceinline__ void lf_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

constexpr uint32_t kLfEmpty = 0xFFFFFFFFu;  // (no node: ids are below n < 2^32)

__global__ void __launch_bounds__(64 * kLfWaves) k_lf_bfs(LfArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_hash[kLfWaves][kLfHashSlots];
    __shared__ uint32_t s_queue[kLfWaves][kLfQueueLds];
    __shared__ uint64_t s_stage[kLfWaves][kLfStage];
    __shared__ uint32_t s_scan[kLfWaves][64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kLfWaves + wv));
    const uint32_t nwaves = gridDim.x * kLfWaves;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t* __restrict__ hs = s_hash[wv];
    uint32_t* __restrict__ lq = s_queue[wv];
    uint64_t* __restrict__ st = s_stage[wv];
    uint32_t* __restrict__ sc = s_scan[wv];
    uint32_t* __restrict__ gq = a.queue + (size_t)wave * a.qstride;  // list entries kLfQueueLds ..
    uint32_t* __restrict__ bm = a.bits + (size_t)wave * a.bstride;   // all zero between two sources
    uint32_t fill = 0;  // staged keys of this wave (wave-uniform)
    unsigned long long visits = 0;  // adjacency entries this wave looked at (wave-uniform)

    auto flush = [&]() {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.count, (unsigned long long)fill);
        base = (unsigned long long)__shfl((long long)base, 0);
        for (uint32_t k = lane; k < fill; k += 64u) {
            const unsigned long long p = base + k;
            if (p < a.cap) a.keys[p] = st[k];
        }
        lf_wave_sync();
        fill = 0;
    };
    // entry i of the wave's list
    auto list_get = [&](uint32_t i) -> uint32_t {
        if (i < (uint32_t)kLfQueueLds) return lq[i];
        const uint32_t g = i - (uint32_t)kLfQueueLds;
        return g < a.qstride ? gq[g] : 0u;
    };
    auto list_put = [&](uint32_t i, uint32_t w) {
        if (i < (uint32_t)kLfQueueLds) {
            lq[i] = w;
        } else {
            const uint32_t g = i - (uint32_t)kLfQueueLds;
            if (g < a.qstride) gq[g] = w;
        }
    };
    // w into the hash set: 1 new, 0 already there, 2 no free slot within the probe limit
    auto hash_insert = [&](uint32_t w) -> int {
        uint32_t slot = (w * 2654435761u) >> (32 - kLfHashBits);
        for (int p = 0; p < kLfProbe; ++p) {
            const uint32_t old = atomicCAS(hs + slot, kLfEmpty, w);
            if (old == kLfEmpty) return 1;
            if (old == w) return 0;
            slot = (slot + 1u) & (uint32_t)(kLfHashSlots - 1);
        }
        return 2;
    };
    auto bits_insert = [&](uint32_t w) -> int {
        const uint32_t bit = 1u << (w & 31u);
        return (atomicOr(bm + (w >> 5), bit) & bit) ? 0 : 1;
    };

    auto hash_clear = [&]() {  // (16 bytes per lane and store)
        const uint4 e4 = make_uint4(kLfEmpty, kLfEmpty, kLfEmpty, kLfEmpty);
        for (uint32_t k = lane; k < (uint32_t)kLfHashSlots / 4u; k += 64u) ((uint4*)hs)[k] = e4;
        lf_wave_sync();
    };
    hash_clear();

    for (uint32_t s = wave; s < a.ns; s += nwaves) {
        const uint32_t u = a.src[s];
        const uint64_t lu = a.lab[u];
        bool in_bits = false;          // the visited set moved to the bitmap (wave-uniform)
        uint32_t lb = 0, le = 1;       // the frontier: entries lb .. le of the list
        if (lane == 0) {
            lq[0] = u;
            hash_insert(u);
        }
        lf_wave_sync();
        for (uint32_t level = 1; level <= a.depth && lb < le; ++level) {
            uint32_t tail = le;  // the list's length (wave-uniform)
            for (uint32_t base = lb; base < le; base += 64u) {
                // 64 nodes of the frontier: their lists' starts and the scan of their lengths
                const bool has = base + lane < le;
                const uint32_t node = has ? list_get(base + lane) : 0u;
                const uint32_t r0 = has ? a.row[node] : 0u;
                const uint32_t dg = has ? a.row[node + 1u] - r0 : 0u;
                uint32_t inc = dg;  // inclusive scan (the degrees of distinct nodes sum to < 2^32)
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t t = (uint32_t)__shfl_up((int)inc, d);
                    if (lane >= (uint32_t)d) inc += t;
                }
                const uint32_t total = (uint32_t)__shfl((int)inc, 63);
                sc[lane] = inc - dg;  // exclusive
                visits += total;
                lf_wave_sync();
                for (uint32_t e0 = 0; e0 < total; e0 += 64u) {
                    const uint32_t e = e0 + lane;
                    const bool act = e < total;
                    // the owner of entry e: the last lane whose exclusive sum is <= e
                    uint32_t o = 0;
                    for (int d = 32; d > 0; d >>= 1)
                        if (sc[o + d] <= e) o += d;
                    const uint32_t osum = sc[o];
                    const uint32_t orow = (uint32_t)__shfl((int)r0, (int)o);
                    const uint32_t w = act ? a.adj[orow + (e - osum)] : 0u;
                    int res = 0;  // 1 new, 0 seen, 2 wants the bitmap
                    if (act) res = in_bits ? bits_insert(w) : hash_insert(w);
                    const uint64_t mnew = __ballot(res == 1);
                    uint32_t nnew = (uint32_t)__popcll(mnew);
                    if (res == 1) list_put(tail + (uint32_t)__popcll(mnew & below), w);
                    lf_wave_sync();
                    tail += nnew;
                    bool isnew = res == 1;
                    if (!in_bits && (__ballot(res == 2) != 0ull || tail > (uint32_t)kLfHashFill)) {
                        // the visited set moves to the bitmap: every node of the list, then the
                        // lanes the hash set turned away
                        for (uint32_t i = lane; i < tail; i += 64u) bits_insert(list_get(i));
                        in_bits = true;
                        lf_wave_sync();
                        const int r2 = res == 2 ? bits_insert(w) : 0;
                        const uint64_t m2 = __ballot(r2 == 1);
                        if (r2 == 1) list_put(tail + (uint32_t)__popcll(m2 & below), w);
                        lf_wave_sync();
                        tail += (uint32_t)__popcll(m2);
                        isnew = isnew || r2 == 1;
                    }
                    if (level >= 2u) {
                        bool emit = isnew && w > u;
                        if (emit) {
                            const uint64_t lw = a.lab[w];
                            emit = lw != a.ignore && (a.mode == kLfModeAll || (a.mode == kLfModeSame) == (lw == lu));
                        }
                        const uint64_t me = __ballot(emit);
                        if (me != 0ull) {
                            const uint32_t ne = (uint32_t)__popcll(me);
                            if (fill + ne > (uint32_t)kLfStage) flush();
                            if (emit) st[fill + (uint32_t)__popcll(me & below)] = ((uint64_t)u << a.b) | (uint64_t)w;
                            lf_wave_sync();
                            fill += ne;
                        }
                    }
                }
                lf_wave_sync();  // (sc is rewritten by the next 64 nodes)
            }
            lb = le;
            le = tail;
        }
        // the visited set is emptied for the next source: the bitmap by the list, the hash set whole
        if (in_bits) {
            for (uint32_t i = lane; i < le; i += 64u) atomicExch(bm + (list_get(i) >> 5), 0u);
        }
        hash_clear();
    }
    if (fill) flush();
    if (lane == 0 && visits) atomicAdd(a.visits, visits);
}

__global__ void __launch_bounds__(256) k_lf_unpack(const uint64_t* __restrict__ keys, int64_t n, int b,
                                                   uint64_t* __restrict__ out) {
    const uint64_t mask = (1ull << b) - 1ull;  // (b <= 32)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[i];
        ((ulonglong2*)out)[i] = make_ulonglong2(k >> b, k & mask);
    }
}

}  // namespace ctws
