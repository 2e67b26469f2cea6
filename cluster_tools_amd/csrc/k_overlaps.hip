// k_overlaps.hip — NodeLabelWorkflow on gfx950: the overlaps of two uint64 label arrays.
//
// Reference: node_labels/block_node_labels.py:130-170 (`_labels_for_block`:
// `ndist.computeAndSerializeLabelOverlaps(nodes, labels, ..., withIgnoreLabel, ignoreLabel)`): for
// every pair (node, label) that occurs at some voxel the number of such voxels, without the voxels
// whose label is the ignore label.
//
//   k_ov_pairs  one pass over both arrays, 16 B per voxel.  Only the voxel correspondence matters,
//               so the arrays are walked flat in words of 64 voxels, a wave per word.  Labels are
//               spatially coherent: a wave merges the runs of equal (node, label) pairs among its
//               64 voxels (the run of k_eval_add, which may cross a row end) and only the run
//               heads are emitted, with the run length as the weight (rag_run_len).  The emits
//               are staged per wave in LDS and appended with one device-scope atomicAdd per full
//               stage, as in k_rag_pairs; the counter keeps counting past the buffer's capacity
//               and nothing is written there, so the host re-runs with the counted size.
//   the rows    come from the path behind ctws_unique_pairs_u64 (k_rag.hip): ids -> ranks in the
//               sorted table of all values of both sides, radix sort of rank(node) << b |
//               rank(label), sum of the weights of equal keys.  One table for both sides keeps
//               the key order the lexicographic (node, label) order.
//   k_ov_rows   (pairs m x 2, sums m) -> rows m x 3.
// Limits (those of that path): fewer than 2^31 voxels, 2^30 emitted runs and 2^32 distinct values
// (node ids and label ids together) per call.
#include "ctws_kernels.h"

namespace ctws {

constexpr int kOvStage = 256;  // staged emits per wave (a step emits at most 64)

__global__ void __launch_bounds__(256) k_ov_pairs(OvArgs a) {
    __shared__ ulonglong2 sp[4][kOvStage];
    __shared__ uint8_t sw[4][kOvStage];  // (a run is at most 64 long)
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t W = (a.n + 63u) >> 6;  // (a.n < 2^31)
    const uint64_t below = (1ull << lane) - 1ull;
    ulonglong2* __restrict__ sp_w = sp[wv];
    uint8_t* __restrict__ sw_w = sw[wv];
    uint32_t fill = 0;  // staged emits of this wave (wave-uniform)
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
    for (uint32_t w = wave0; w < W; w += nwaves) {
        const uint32_t i = (w << 6) + lane;
        const bool in = i < a.n;
        const uint64_t u = in ? a.nodes[i] : 0ull;
        const uint64_t l = in ? a.labels[i] : 0ull;
        const bool use = in && !(a.with_ignore && l == a.ignore_label);
        const uint64_t um = __ballot(use);
        if (um == 0ull) continue;  // nothing counted in this word
        // a lane heads a run when its predecessor is not counted or holds another pair
        const uint64_t up = (uint64_t)__shfl_up((long long)u, 1), lp = (uint64_t)__shfl_up((long long)l, 1);
        const bool prev = lane != 0 && ((um >> (lane - 1u)) & 1ull);
        const bool head = use && (!prev || up != u || lp != l);
        const uint64_t hm = __ballot(head);
        const uint32_t ne = (uint32_t)__popcll(hm);
        if (fill + ne > (uint32_t)kOvStage) flush();
        if (head) {
            const uint32_t k = fill + (uint32_t)__popcll(hm & below);
            sp_w[k] = make_ulonglong2(u, l);
            sw_w[k] = (uint8_t)rag_run_len(um & ~hm, lane);
        }
        __builtin_amdgcn_wave_barrier();
        fill += ne;
    }
    if (fill) flush();
}

__global__ void __launch_bounds__(256) k_ov_rows(const uint64_t* __restrict__ pairs, const uint64_t* __restrict__ sums,
                                                 int64_t m, uint64_t* __restrict__ rows) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const ulonglong2 p = ((const ulonglong2*)pairs)[i];
        rows[3 * i] = p.x;
        rows[3 * i + 1] = p.y;
        rows[3 * i + 2] = sums[i];
    }
}

}  // namespace ctws
