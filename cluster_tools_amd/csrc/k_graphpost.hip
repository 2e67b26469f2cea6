// k_graphpost.hip — the graph-based half of the postprocessing on gfx950: graph connected components
// and the seeded graph watershed over the merged graph's edge table.
//
// References: postprocess/graph_connected_components.py:104-121
// (`ndist.connectedComponentsFromNodes` + `relabelConsecutive`) and
// postprocess/graph_watershed_assignments.py:152-178 (`nifty.graph.edgeWeightedWatershedsSegmentation`);
// nifty is not available, the semantics are decided in DESIGN.md 3.13.
//
// Components
//   k_gp_init      parent[i] = i.
//   k_gp_union     one thread per edge: rows with an id >= n are counted and skipped; an edge whose
//                  ends carry the same non-zero assignment unites them.  A union hooks the LARGER
//                  root under the smaller id with atomicMin, so parent[x] <= x always holds (no
//                  cycle can form) and every root ends up as its component's smallest node.  When
//                  the atomicMin finds that the node was no root any more, the pair (what it
//                  pointed to, the other root) is united instead: both ids are below the node's, so
//                  the retries end.  Lock-free: no thread waits for another.
//   k_gp_compress  parent[i] = root of i (a walk down strictly descending ids).
//   k_gp_cc_flag   flag[i] = i is a root with a non-zero assignment; an exclusive scan of the flags
//                  numbers the components by their smallest node ...
//   k_gp_cc_write  ... and out[i] = 1 + num[parent[i]], or 0 for assignment 0.
//
// Watershed (seeded Boruvka rounds on a total order; equal to the sequential priority-queue flood
// with ties ordered by edge index)
//   k_gp_keys      per edge the order-preserving 64-bit image of its weight (-0.0 as 0.0; NaN and
//                  ids >= n are counted) and its index; ONE stable radix sort of the pairs then
//                  gives every edge its rank, and k_gp_sorted_ends stores the ends in rank order
//                  as 32-bit ids: position = rank.
//   a round:
//   k_gp_offer     one thread per edge in rank order.  An edge inside one component or between two
//                  seeded components is dead for good and marks itself (u := v) so that later
//                  rounds skip its gathers; any other edge offers its rank to each unseeded side
//                  (atomicMin on best[root]).
//   k_gp_hook      every unseeded root with an offer points to the root across its best edge; of
//                  two unseeded roots that chose the same edge the smaller id stays root.  Reads
//                  the parents of the round's start, writes a second array: no thread reads what
//                  another writes.  Resets best[] for the next round and counts the hooks.
//   k_gp_jump      pointer jumping, in place (whatever a thread reads is an ancestor): up to four
//                  jumps per node and pass; a node that still is not at a root sets the pass's
//                  flag.  The host repeats passes until a flag stays clear, at most kGpMaxIters.
//   Seeded nodes never hook, so they stay roots and a component's label is its root's seed:
//   k_gp_ws_write  out[i] = seeds[parent[i]].
//   The host stops when a round hooked nothing, at most kGpMaxIters rounds (a round at least
//   halves the unseeded components that still have an outgoing edge).
// Relabel (first appearance over the node index, from 1, zeros kept): a stable sort of
//   (label, node) puts every label's first node at the head of its run; k_gp_rl_heads flags those
//   nodes, a scan numbers them, and k_gp_rl_write finds its run's head by a binary search.
// Integer arithmetic and integer atomics only; the results do not depend on the atomics' order.
// Node ids and ranks are 32-bit (n < 2^32, m < 2^32); loop counters are 64-bit.
#include "ctws_kernels.h"

namespace ctws {

namespace {
constexpr uint32_t kGpNone = 0xFFFFFFFFu;  // no offer (ranks are below m < 2^32)

__device__ __forceinline__ uint32_t gp_ld(const uint32_t* q) {
    return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t gp_root(const uint32_t* parent, uint32_t x) {
    for (uint32_t p = gp_ld(parent + x); p != x; p = gp_ld(parent + x)) x = p;  // (p < x: it ends)
    return x;
}
}  // namespace

#define GP_LOOP(i, n)                                                                       \
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (uint64_t)(n); \
         i += (uint64_t)gridDim.x * blockDim.x)

__global__ void __launch_bounds__(256) k_gp_init(uint32_t* __restrict__ parent, uint32_t* __restrict__ best, uint64_t n) {
    GP_LOOP(i, n) {
        parent[i] = (uint32_t)i;
        if (best) best[i] = kGpNone;
    }
}

__global__ void __launch_bounds__(256) k_gp_union(const uint64_t* __restrict__ edges, uint64_t m, uint64_t n,
                                                  const uint64_t* __restrict__ assign, uint32_t* __restrict__ parent,
                                                  unsigned long long* __restrict__ bad) {
    GP_LOOP(i, m) {
        const ulonglong2 e = ((const ulonglong2*)edges)[i];
        if (e.x >= n || e.y >= n) {
            atomicAdd(bad + kGpBadId, 1ull);
            continue;
        }
        const uint64_t a = assign[e.x];
        if (a == 0ull || a != assign[e.y]) continue;
        uint32_t u = gp_root(parent, (uint32_t)e.x), v = gp_root(parent, (uint32_t)e.y);
        while (u != v) {
            const uint32_t hi = u > v ? u : v, lo = u > v ? v : u;
            const uint32_t old = atomicMin(parent + hi, lo);
            if (old == hi) break;  // hi was a root and now hangs under lo
            // hi pointed to old < hi: old and lo are to be one component (both below hi)
            u = gp_root(parent, old);
            v = gp_root(parent, lo);
        }
    }
}

__global__ void __launch_bounds__(256) k_gp_compress(uint32_t* __restrict__ parent, uint64_t n) {
    GP_LOOP(i, n) {
        const uint32_t r = gp_root(parent, (uint32_t)i);
        if (r != (uint32_t)i) parent[i] = r;  // (a root's word is never written)
    }
}

__global__ void __launch_bounds__(256) k_gp_cc_flag(const uint32_t* __restrict__ parent, const uint64_t* __restrict__ assign,
                                                    uint64_t n, uint32_t* __restrict__ flag) {
    GP_LOOP(i, n) flag[i] = (parent[i] == (uint32_t)i && assign[i] != 0ull) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_gp_cc_write(const uint32_t* __restrict__ parent, const uint64_t* __restrict__ assign,
                                                     const uint32_t* __restrict__ num, uint64_t n, uint64_t* __restrict__ out) {
    GP_LOOP(i, n) out[i] = assign[i] == 0ull ? 0ull : 1ull + (uint64_t)num[parent[i]];
}

__global__ void __launch_bounds__(256) k_gp_keys(const uint64_t* __restrict__ edges, const double* __restrict__ weights,
                                                 uint64_t m, uint64_t n, uint64_t* __restrict__ keys,
                                                 uint32_t* __restrict__ idx, unsigned long long* __restrict__ bad) {
    GP_LOOP(i, m) {
        const ulonglong2 e = ((const ulonglong2*)edges)[i];
        if (e.x >= n || e.y >= n) atomicAdd(bad + kGpBadId, 1ull);
        double w = weights[i];
        if (w != w) atomicAdd(bad + kGpBadNan, 1ull);
        if (w == 0.0) w = 0.0;  // -0.0 is 0.0: a tie, decided by the index
        const uint64_t b = (uint64_t)__double_as_longlong(w);
        keys[i] = (b >> 63) ? ~b : (b | 0x8000000000000000ull);  // ascending as float64 ascends
        idx[i] = (uint32_t)i;
    }
}

// (the rows passed k_gp_keys: every id is below n < 2^32)
__global__ void __launch_bounds__(256) k_gp_sorted_ends(const uint64_t* __restrict__ edges, const uint32_t* __restrict__ order,
                                                        uint64_t m, uint32_t* __restrict__ su, uint32_t* __restrict__ sv) {
    GP_LOOP(r, m) {
        const ulonglong2 e = ((const ulonglong2*)edges)[order[r]];
        su[r] = (uint32_t)e.x;
        sv[r] = (uint32_t)e.y;
    }
}

__global__ void __launch_bounds__(256) k_gp_offer(uint32_t* __restrict__ su, const uint32_t* __restrict__ sv, uint64_t m,
                                                  const uint32_t* __restrict__ parent, const uint64_t* __restrict__ seeds,
                                                  uint32_t* __restrict__ best) {
    GP_LOOP(r, m) {
        const uint32_t u = su[r], v = sv[r];
        if (u == v) continue;  // dead
        const uint32_t cu = parent[u], cv = parent[v];  // (compressed: the roots)
        const bool fu = seeds[cu] != 0ull, fv = seeds[cv] != 0ull;
        if (cu == cv || (fu && fv)) {
            su[r] = v;
            continue;
        }
        if (!fu) atomicMin(best + cu, (uint32_t)r);
        if (!fv) atomicMin(best + cv, (uint32_t)r);
    }
}

__global__ void __launch_bounds__(256) k_gp_hook(const uint32_t* __restrict__ su, const uint32_t* __restrict__ sv,
                                                 const uint32_t* __restrict__ parent, const uint64_t* __restrict__ seeds,
                                                 const uint32_t* __restrict__ best, uint32_t* __restrict__ next, uint64_t n,
                                                 unsigned long long* __restrict__ hooks) {
    GP_LOOP(i, n) {
        const uint32_t c = (uint32_t)i;
        uint32_t p = parent[c];
        const uint32_t r = best[c];
        if (r != kGpNone) {  // (only unseeded roots get offers)
            const uint32_t cu = parent[su[r]], cv = parent[sv[r]];
            const uint32_t o = cu == c ? cv : cu;
            if (!(seeds[o] == 0ull && best[o] == r && c < o)) {
                p = o;
                atomicAdd(hooks, 1ull);
            }
        }
        next[c] = p;
    }
}

// (after k_gp_hook: best[] is read by no one until the next round's offers)
__global__ void __launch_bounds__(256) k_gp_jump(uint32_t* __restrict__ parent, uint32_t* __restrict__ best, uint64_t n,
                                                 unsigned long long* __restrict__ open) {
    GP_LOOP(i, n) {
        if (best) best[i] = kGpNone;
        const uint32_t p0 = gp_ld(parent + i);
        uint32_t p = p0, q = gp_ld(parent + p);
        for (int k = 0; k < 4 && q != p; ++k) {
            p = q;
            q = gp_ld(parent + p);
        }
        if (p != p0) parent[i] = p;
        if (q != p) atomicOr(open, 1ull);
    }
}

__global__ void __launch_bounds__(256) k_gp_ws_write(const uint32_t* __restrict__ parent, const uint64_t* __restrict__ seeds,
                                                     uint64_t n, uint64_t* __restrict__ out) {
    GP_LOOP(i, n) out[i] = seeds[parent[i]];
}

__global__ void __launch_bounds__(256) k_gp_rl_keys(const uint64_t* __restrict__ lab, uint64_t n, uint64_t* __restrict__ keys,
                                                    uint32_t* __restrict__ idx, uint32_t* __restrict__ flag) {
    GP_LOOP(i, n) {
        keys[i] = lab[i];
        idx[i] = (uint32_t)i;
        flag[i] = 0u;
    }
}

__global__ void __launch_bounds__(256) k_gp_rl_heads(const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ sidx,
                                                     uint64_t n, uint32_t* __restrict__ flag) {
    GP_LOOP(p, n) {
        const uint64_t k = skeys[p];
        if (k != 0ull && (p == 0 || skeys[p - 1] != k)) flag[sidx[p]] = 1u;
    }
}

__global__ void __launch_bounds__(256) k_gp_rl_write(const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ sidx,
                                                     const uint32_t* __restrict__ num, uint64_t n, uint64_t* __restrict__ out) {
    GP_LOOP(p, n) {
        const uint64_t k = skeys[p];
        uint64_t v = 0ull;
        if (k != 0ull) {
            uint64_t lo = 0, hi = p;  // the first position of k's run lies in [lo, hi]
            while (lo < hi) {
                const uint64_t mid = (lo + hi) >> 1;
                if (skeys[mid] < k) lo = mid + 1;
                else hi = mid;
            }
            v = 1ull + (uint64_t)num[sidx[lo]];
        }
        out[sidx[p]] = v;
    }
}

}  // namespace ctws
