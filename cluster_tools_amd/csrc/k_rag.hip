// k_rag.hip — GraphWorkflow on gfx950: the region adjacency graph of a block of uint64 labels.
//
// Reference: graph/initial_sub_graphs.py:106-120 (`ndist.computeMergeableRegionGraph` per block,
// increaseRoi=True), merge_sub_graphs.py:133-158 (`ndist.mergeSubgraphs`: the union of the
// children's node and edge tables).  The edges of a block are the set of (min(u, v), max(u, v))
// over all face-adjacent voxel pairs with u != v (and u, v != 0 under ignore_label), sorted.
//
//   k_rag_pairs   one pass over the block, 8 B per voxel.  A wave owns a row and walks it in words
//                 of 64 voxels: a lane has its voxel, gets the +x neighbour from the next lane
//                 (lane 63 loads it) and the +y / +z neighbours by coalesced loads of the two
//                 adjacent rows.  Inside a fragment all three comparisons are equal, so one
//                 ballot lets the wave skip everything else.  On the y and z axes a boundary
//                 surface gives runs of the same (u, v) along x: a lane emits only where its
//                 pair differs from its predecessor lane's, with the run length as the weight
//                 (the head and ballot idea of k_sf_member), so the counts stay exact.  A
//                 wave stages its emits in its own slice of LDS (kRagStage entries) and
//                 appends a full stage with ONE device-scope atomicAdd and coalesced stores:
//                 nearly every word of a row crosses a fragment border, and one atomic per
//                 wave and step on a single counter word would bound the pass far below the
//                 stream.  The counter keeps counting past the buffer's capacity and nothing
//                 is written there, so the host can re-run with a buffer of the counted size.
//                 The node table comes from the same pass: a voxel whose +x, +y and +z
//                 neighbours all differ from it (or lie outside the block) emits its id, staged
//                 and appended the same way.  Every connected piece of a fragment has such a
//                 voxel (its last one in scan order), so the sorted unique of these few ids is
//                 np.unique of the block, and the labels are not read a second time.
//   k_pair_keys   (u, v) -> rank(u) << b | rank(v): binary searches in a sorted table of the
//                 endpoint values (the block's node table), b bits per rank.
//   sort_pairs_u64 / reduce_by_key_sum_u64  radix sort of (key, weight) over the 2 b key bits
//                 and the sum of the weights of equal keys (k_prims.hip, device-wide).
//   k_pair_unpack key -> (table[key >> b], table[key & mask]).
// Index arithmetic inside a block is 32-bit (a block holds fewer than 2^31 voxels) and there is
// no division per voxel: one 32-bit division per row, on a wave-uniform value.
#include "ctws_kernels.h"

namespace ctws {

constexpr int kRagStage = 512;      // staged emits per wave (a step emits at most 3 * 64)
constexpr int kRagNodeStage = 128;  // staged node emits per wave (a step emits at most 64)

__global__ void __launch_bounds__(256) k_rag_pairs(RagArgs a) {
    __shared__ ulonglong2 sp[4][kRagStage];
    __shared__ uint8_t sw[4][kRagStage];  // (a run is at most 64 long)
    __shared__ uint64_t sn[4][kRagNodeStage];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t rows = a.nz * a.ny, W = (a.nx + 63u) >> 6;
    const uint32_t sy = a.nx, sz = a.ny * a.nx;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint32_t pl = (lane - 1u) & 63u;  // the predecessor lane (unused by lane 0)
    ulonglong2* __restrict__ sp_w = sp[wv];
    uint8_t* __restrict__ sw_w = sw[wv];
    uint64_t* __restrict__ sn_w = sn[wv];
    uint32_t fill = 0, nfill = 0;  // staged emits / node emits of this wave (wave-uniform)
    // the wave's staged emits -> the pair buffer: one atomicAdd, coalesced stores
    auto flush = [&]() {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.count, (unsigned long long)fill);
        base = (unsigned long long)__shfl((long long)base, 0);
        for (uint32_t k = lane; k < fill; k += 64u) {
            const unsigned long long p = base + k;
            if (p < a.cap) {
                ((ulonglong2*)a.pairs)[p] = sp_w[k];
                a.weights[p] = (uint64_t)sw_w[k];
            }
        }
        __builtin_amdgcn_wave_barrier();
        fill = 0;
    };
    auto flush_nodes = [&]() {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.ncount, (unsigned long long)nfill);
        base = (unsigned long long)__shfl((long long)base, 0);
        for (uint32_t k = lane; k < nfill; k += 64u) {
            const unsigned long long p = base + k;
            if (p < a.ncap) a.nodes[p] = sn_w[k];
        }
        __builtin_amdgcn_wave_barrier();
        nfill = 0;
    };
    for (uint32_t r = wave0; r < rows; r += nwaves) {
        const uint32_t z = r / a.ny, y = r - z * a.ny;
        const bool hy = y + 1u < a.ny, hz = z + 1u < a.nz;
        const uint32_t rb = r * a.nx;
        for (uint32_t w = 0; w < W; ++w) {
            const uint32_t x = (w << 6) + lane;
            const bool in = x < a.nx, hx = x + 1u < a.nx;
            const uint32_t i = rb + x;
            const uint64_t v = in ? a.lab[i] : 0ull;
            const uint64_t vy = in && hy ? a.lab[i + sy] : 0ull;
            const uint64_t vz = in && hz ? a.lab[i + sz] : 0ull;
            const uint64_t vn = (uint64_t)__shfl_down((long long)v, 1);
            const uint64_t vx = lane == 63 && hx ? a.lab[i + 1u] : vn;
            const bool nz0 = !a.ignore || v != 0ull;
            const bool dx = hx && v != vx && nz0 && (!a.ignore || vx != 0ull);
            const bool dy = in && hy && v != vy && nz0 && (!a.ignore || vy != 0ull);
            const bool dz = in && hz && v != vz && nz0 && (!a.ignore || vz != 0ull);
            // a voxel whose three upper neighbours all differ (or lie outside) emits its id as a
            // node: the last voxel of every connected piece of a fragment is one
            const bool corner = in && nz0 && (!hx || v != vx) && (!hy || v != vy) && (!hz || v != vz);
            const uint64_t mx = __ballot(dx), my = __ballot(dy), mz = __ballot(dz), mc = __ballot(corner);
            if ((mx | my | mz | mc) == 0ull) continue;  // a fragment's interior: nothing to emit
            if (mc) {
                const uint32_t nc = (uint32_t)__popcll(mc);
                if (nfill + nc > (uint32_t)kRagNodeStage) flush_nodes();
                if (corner) sn_w[nfill + (uint32_t)__popcll(mc & below)] = v;
                __builtin_amdgcn_wave_barrier();
                nfill += nc;
                if ((mx | my | mz) == 0ull) continue;
            }
            // run heads along x on the y and z axes (bit l of meq: lanes l and l + 1 hold the same id)
            const uint64_t meq = __ballot(v == vn);
            const uint64_t vyp = (uint64_t)__shfl_up((long long)vy, 1);
            const uint64_t vzp = (uint64_t)__shfl_up((long long)vz, 1);
            const bool first = lane == 0;
            const bool same = (meq >> pl) & 1ull;
            const bool hdy = dy && (first || !((my >> pl) & 1ull) || !same || vy != vyp);
            const bool hdz = dz && (first || !((mz >> pl) & 1ull) || !same || vz != vzp);
            const uint64_t ey = __ballot(hdy), ez = __ballot(hdz);
            const uint32_t nxe = (uint32_t)__popcll(mx), nye = (uint32_t)__popcll(ey), nze = (uint32_t)__popcll(ez);
            if (fill + nxe + nye + nze > (uint32_t)kRagStage) flush();  // (a step emits at most 192)
            if (dx) {
                const uint32_t k = fill + (uint32_t)__popcll(mx & below);
                sp_w[k] = make_ulonglong2(v < vx ? v : vx, v < vx ? vx : v);
                sw_w[k] = (uint8_t)1;
            }
            if (hdy) {
                const uint32_t k = fill + nxe + (uint32_t)__popcll(ey & below);
                sp_w[k] = make_ulonglong2(v < vy ? v : vy, v < vy ? vy : v);
                sw_w[k] = (uint8_t)rag_run_len(my & ~ey, lane);
            }
            if (hdz) {
                const uint32_t k = fill + nxe + nye + (uint32_t)__popcll(ez & below);
                sp_w[k] = make_ulonglong2(v < vz ? v : vz, v < vz ? vz : v);
                sw_w[k] = (uint8_t)rag_run_len(mz & ~ez, lane);
            }
            __builtin_amdgcn_wave_barrier();
            fill += nxe + nye + nze;
        }
    }
    if (fill) flush();
    if (nfill) flush_nodes();
}

// first index with tab[idx] >= v (tab ascending and holding v)
__device__ __forceinline__ uint64_t rag_rank(const uint64_t* __restrict__ tab, int64_t nt, uint64_t v) {
    int64_t lo = 0, hi = nt;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (tab[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return (uint64_t)lo;
}

// keys[i] = rank(u_i) << b | rank(v_i); a value missing from the table is counted
__global__ void __launch_bounds__(256) k_pair_keys(const uint64_t* __restrict__ pairs, int64_t n,
                                                   const uint64_t* __restrict__ tab, int64_t nt, int b,
                                                   uint64_t* __restrict__ keys, unsigned long long* __restrict__ missing) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const ulonglong2 p = ((const ulonglong2*)pairs)[i];
        const uint64_t ru = rag_rank(tab, nt, p.x), rv = rag_rank(tab, nt, p.y);
        if (ru >= (uint64_t)nt || rv >= (uint64_t)nt || tab[ru] != p.x || tab[rv] != p.y) {
            atomicAdd(missing, 1ull);
            keys[i] = 0ull;
        } else {
            keys[i] = (ru << b) | rv;
        }
    }
}

__global__ void __launch_bounds__(256) k_pair_ones(uint64_t* __restrict__ w, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        w[i] = 1ull;
}

__global__ void __launch_bounds__(256) k_pair_unpack(const uint64_t* __restrict__ keys, int64_t n,
                                                     const uint64_t* __restrict__ tab, int b,
                                                     uint64_t* __restrict__ out) {
    const uint64_t mask = (1ull << b) - 1ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = keys[i];
        ((ulonglong2*)out)[i] = make_ulonglong2(tab[k >> b], tab[k & mask]);
    }
}

}  // namespace ctws
