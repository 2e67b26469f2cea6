// ctws_graphpost.cpp — host side of libctws.so: graph components and the graph watershed.
#include "ctws_host.h"

using namespace ctws;

// ---- ConnectedComponentsWorkflow, SizeFilterAndGraphWatershedWorkflow: graph components and the
// ---- seeded graph watershed over the merged graph's edge table (k_graphpost.hip) ----
namespace {
// the counter block: the edge checks' words, and a line for a round's hooks and a pass's open flag
enum GpWord : size_t { kGpWordHooks = 16, kGpWordOpen = 17, kGpWords = 32 };

unsigned gp_grid(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 8192); }

// the checks both calls share; *done: nothing is left to do (no node)
int gp_begin(ctws_handle* h, const char* what, const void* edges, int64_t m, const void* nodes, int64_t n, const void* out,
             bool* done) {
    int r;
    *done = false;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    if (m < 0 || n < 0 || (m > 0 && !edges) || (n > 0 && (!nodes || !out))) {
        h->err = std::string(what) + ": bad arguments (an edge table for n_edges > 0, node arrays for n_nodes > 0)";
        return CTWS_EINVAL;
    }
    if (n >= (1ll << 32) || m >= (1ll << 32)) {
        h->err = std::string(what) + ": 2^32 or more nodes or edges (node ids and edge ranks are 32-bit)";
        return CTWS_EUNSUPPORTED;
    }
    if (n == 0) {
        if (m > 0) {
            h->err = std::string(what) + ": " + std::to_string(m) + " rows hold an id >= n_nodes (0)";
            return CTWS_EINVAL;
        }
        *done = true;
    }
    return CTWS_OK;
}

// the edge checks' counters of a call; the stream has drained when this returns
int gp_edge_check(ctws_handle* h, const char* what, unsigned long long* red, int64_t n) {
    unsigned long long w[2];
    HIPCHK(hipMemcpyAsync(w, red, sizeof(w), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (w[kGpBadId] || w[kGpBadNan]) {
        h->err = std::string(what) + ": " + std::to_string(w[kGpBadId]) + " rows hold an id >= n_nodes (" +
                 std::to_string(n) + "), " + std::to_string(w[kGpBadNan]) + " weights are NaN";
        return CTWS_EINVAL;
    }
    return CTWS_OK;
}

// lab (n, on the device) renumbered in place by first appearance over the index, from 1, zeros kept
int gp_relabel(ctws_handle* h, uint64_t* lab, int64_t n) {
    int r;
    if ((r = grow(h, h->gp_keys, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_skeys, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_idx, sizeof(uint32_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_sidx, sizeof(uint32_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_best, sizeof(uint32_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_num, sizeof(uint32_t) * (size_t)n)) != CTWS_OK) return r;
    size_t tb_sort = 0, tb_scan = 0;
    HIPCHK(sort_pairs_u64_u32(nullptr, tb_sort, nullptr, nullptr, nullptr, nullptr, n, h->stream));
    HIPCHK(exclusive_sum_u32(nullptr, tb_scan, nullptr, nullptr, n, h->stream));
    if ((r = grow(h, h->prim_tmp, std::max(tb_sort, tb_scan))) != CTWS_OK) return r;
    uint64_t *keys = (uint64_t*)h->gp_keys.p, *skeys = (uint64_t*)h->gp_skeys.p;
    uint32_t *idx = (uint32_t*)h->gp_idx.p, *sidx = (uint32_t*)h->gp_sidx.p;
    uint32_t *flag = (uint32_t*)h->gp_best.p, *num = (uint32_t*)h->gp_num.p;
    const unsigned gn = gp_grid(n);
    k_gp_rl_keys<<<gn, 256, 0, h->stream>>>(lab, (uint64_t)n, keys, idx, flag);
    HIPCHK(sort_pairs_u64_u32(h->prim_tmp.p, tb_sort, keys, skeys, idx, sidx, n, h->stream));
    k_gp_rl_heads<<<gn, 256, 0, h->stream>>>(skeys, sidx, (uint64_t)n, flag);
    HIPCHK(exclusive_sum_u32(h->prim_tmp.p, tb_scan, flag, num, n, h->stream));
    k_gp_rl_write<<<gn, 256, 0, h->stream>>>(skeys, sidx, num, (uint64_t)n, lab);
    LAUNCHCHK();
    return CTWS_OK;
}

int graph_components(ctws_handle* h, const uint64_t* edges, int64_t m, const uint64_t* assignments, int64_t n,
                     uint64_t* out, bool dev) {
    const char* what = "graph components";
    int r;
    bool done;
    if (!h) return CTWS_EINVAL;
    if ((r = gp_begin(h, what, edges, m, assignments, n, out, &done)) != CTWS_OK || done) return r;
    const uint64_t *de = nullptr, *da;
    if (m > 0 && (r = stage_in(h, h->gp_edges, edges, 2 * sizeof(uint64_t) * (size_t)m, dev, &de)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->gp_in, assignments, sizeof(uint64_t) * (size_t)n, dev, &da)) != CTWS_OK) return r;
    const size_t nb = sizeof(uint32_t) * (size_t)n;
    if ((r = grow(h, h->gp_red, kGpWords * sizeof(uint64_t))) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_parent, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_best, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_num, nb)) != CTWS_OK) return r;
    size_t tb_scan = 0;
    HIPCHK(exclusive_sum_u32(nullptr, tb_scan, nullptr, nullptr, n, h->stream));
    if ((r = grow(h, h->prim_tmp, tb_scan)) != CTWS_OK) return r;
    unsigned long long* red = (unsigned long long*)h->gp_red.p;
    uint32_t *parent = (uint32_t*)h->gp_parent.p, *flag = (uint32_t*)h->gp_best.p, *num = (uint32_t*)h->gp_num.p;
    const unsigned gn = gp_grid(n);
    record(h, 0);
    k_gp_init<<<gn, 256, 0, h->stream>>>(parent, nullptr, (uint64_t)n);
    if (m > 0) {  // (no edge: no edge kernel, every labelled node is a component)
        HIPCHK(hipMemsetAsync(red, 0, kGpWords * sizeof(uint64_t), h->stream));
        k_gp_union<<<gp_grid(m), 256, 0, h->stream>>>(de, (uint64_t)m, (uint64_t)n, da, parent, red);
        LAUNCHCHK();
        if ((r = gp_edge_check(h, what, red, n)) != CTWS_OK) return r;  // (before anything is written to out)
        k_gp_compress<<<gn, 256, 0, h->stream>>>(parent, (uint64_t)n);
    }
    record(h, 1);
    uint64_t* dout;
    const size_t out_bytes = sizeof(uint64_t) * (size_t)n;
    if ((r = out_begin(h, h->gp_out, out, out_bytes, dev, &dout)) != CTWS_OK) return r;
    k_gp_cc_flag<<<gn, 256, 0, h->stream>>>(parent, da, (uint64_t)n, flag);
    HIPCHK(exclusive_sum_u32(h->prim_tmp.p, tb_scan, flag, num, n, h->stream));
    k_gp_cc_write<<<gn, 256, 0, h->stream>>>(parent, da, num, (uint64_t)n, dout);
    LAUNCHCHK();
    record(h, 2);
    if ((r = out_end(h, out, dout, out_bytes, dev)) != CTWS_OK) return r;
    stage_time(h, "gc_union", 0, 1);
    stage_time(h, "gc_number", 1, 2);
    return CTWS_OK;
}

int graph_watershed(ctws_handle* h, const uint64_t* edges, const double* weights, int64_t m, const uint64_t* seeds,
                    int64_t n, int relabel, uint64_t* out, bool dev) {
    const char* what = "graph watershed";
    int r;
    bool done;
    if (!h) return CTWS_EINVAL;
    if ((r = gp_begin(h, what, edges, m, seeds, n, out, &done)) != CTWS_OK || done) return r;
    if (m > 0 && !weights) {
        h->err = "graph watershed: bad arguments (a weight per edge for n_edges > 0)";
        return CTWS_EINVAL;
    }
    if ((const void*)out == (const void*)seeds) {
        h->err = "graph watershed: out is the seed array (a node reads its root's seed while others are written)";
        return CTWS_EINVAL;
    }
    const uint64_t *de, *ds;
    const double* dw;
    if ((r = stage_in(h, h->gp_in, seeds, sizeof(uint64_t) * (size_t)n, dev, &ds)) != CTWS_OK) return r;
    uint64_t* dout;
    const size_t out_bytes = sizeof(uint64_t) * (size_t)n;
    if ((r = out_begin(h, h->gp_out, out, out_bytes, dev, &dout)) != CTWS_OK) return r;
    const unsigned gn = gp_grid(n);
    int rounds = 0, passes = 0;
    record(h, 0);
    if (m == 0) {  // no edge: no edge kernel, the seeds are the result
        if (dout != ds) HIPCHK(hipMemcpyAsync(dout, ds, out_bytes, hipMemcpyDeviceToDevice, h->stream));
        record(h, 1);
        record(h, 2);
    } else {
        if ((r = stage_in(h, h->gp_edges, edges, 2 * sizeof(uint64_t) * (size_t)m, dev, &de)) != CTWS_OK) return r;
        if ((r = stage_in(h, h->gp_w, weights, sizeof(double) * (size_t)m, dev, &dw)) != CTWS_OK) return r;
        const size_t nb = sizeof(uint32_t) * (size_t)n, mb = sizeof(uint32_t) * (size_t)m;
        if ((r = grow(h, h->gp_red, kGpWords * sizeof(uint64_t))) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_parent, nb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_next, nb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_best, nb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_su, mb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_sv, mb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_idx, mb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_sidx, mb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_keys, 2 * mb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_skeys, 2 * mb)) != CTWS_OK) return r;
        size_t tb_sort = 0;
        HIPCHK(sort_pairs_u64_u32(nullptr, tb_sort, nullptr, nullptr, nullptr, nullptr, m, h->stream));
        if ((r = grow(h, h->prim_tmp, tb_sort)) != CTWS_OK) return r;
        unsigned long long* red = (unsigned long long*)h->gp_red.p;
        uint32_t *parent = (uint32_t*)h->gp_parent.p, *next = (uint32_t*)h->gp_next.p, *best = (uint32_t*)h->gp_best.p;
        uint32_t *su = (uint32_t*)h->gp_su.p, *sv = (uint32_t*)h->gp_sv.p;
        const unsigned gm = gp_grid(m);
        // the checks and the ranks: one stable sort of (ordered weight, edge index)
        HIPCHK(hipMemsetAsync(red, 0, kGpWords * sizeof(uint64_t), h->stream));
        k_gp_keys<<<gm, 256, 0, h->stream>>>(de, dw, (uint64_t)m, (uint64_t)n, (uint64_t*)h->gp_keys.p,
                                             (uint32_t*)h->gp_idx.p, red);
        LAUNCHCHK();
        if ((r = gp_edge_check(h, what, red, n)) != CTWS_OK) return r;
        HIPCHK(sort_pairs_u64_u32(h->prim_tmp.p, tb_sort, (const uint64_t*)h->gp_keys.p, (uint64_t*)h->gp_skeys.p,
                                  (const uint32_t*)h->gp_idx.p, (uint32_t*)h->gp_sidx.p, m, h->stream));
        k_gp_sorted_ends<<<gm, 256, 0, h->stream>>>(de, (const uint32_t*)h->gp_sidx.p, (uint64_t)m, su, sv);
        k_gp_init<<<gn, 256, 0, h->stream>>>(parent, best, (uint64_t)n);
        LAUNCHCHK();
        record(h, 1);
        // the rounds: both loops are capped here, and a cap that is reached is an error
        bool fixed = false;
        unsigned long long w[2];
        for (int round = 0; round < kGpMaxIters && !fixed; ++round) {
            HIPCHK(hipMemsetAsync(red + kGpWordHooks, 0, 2 * sizeof(uint64_t), h->stream));
            k_gp_offer<<<gm, 256, 0, h->stream>>>(su, sv, (uint64_t)m, parent, ds, best);
            k_gp_hook<<<gn, 256, 0, h->stream>>>(su, sv, parent, ds, best, next, (uint64_t)n, red + kGpWordHooks);
            k_gp_jump<<<gn, 256, 0, h->stream>>>(next, best, (uint64_t)n, red + kGpWordOpen);
            LAUNCHCHK();
            HIPCHK(hipMemcpyAsync(w, red + kGpWordHooks, sizeof(w), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            if (w[0] == 0ull) {  // no component hooked: next is parent, the forest is final
                fixed = true;
                break;
            }
            ++rounds;
            int p = 1;
            for (; w[1] != 0ull && p < kGpMaxIters; ++p) {
                HIPCHK(hipMemsetAsync(red + kGpWordOpen, 0, sizeof(uint64_t), h->stream));
                k_gp_jump<<<gn, 256, 0, h->stream>>>(next, nullptr, (uint64_t)n, red + kGpWordOpen);
                LAUNCHCHK();
                HIPCHK(hipMemcpyAsync(w + 1, red + kGpWordOpen, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
                HIPCHK(hipStreamSynchronize(h->stream));
            }
            passes += p;
            if (w[1] != 0ull) {
                h->err = "graph watershed: pointer jumping did not reach a fixpoint in " + std::to_string(kGpMaxIters) +
                         " passes (round " + std::to_string(round) + ")";
                return CTWS_EHIP;
            }
            std::swap(parent, next);
        }
        if (!fixed) {
            h->err = "graph watershed: components still hooked after " + std::to_string(kGpMaxIters) + " rounds";
            return CTWS_EHIP;
        }
        record(h, 2);
        k_gp_ws_write<<<gn, 256, 0, h->stream>>>(parent, ds, (uint64_t)n, dout);
        LAUNCHCHK();
    }
    if (relabel && (r = gp_relabel(h, dout, n)) != CTWS_OK) return r;
    record(h, 3);
    if ((r = out_end(h, out, dout, out_bytes, dev)) != CTWS_OK) return r;
    stage_time(h, "gw_sort", 0, 1);
    stage_time(h, "gw_rounds_ms", 1, 2);
    stage_time(h, "gw_write", 2, 3);
    add_timing(h, "gw_rounds", (float)rounds);
    add_timing(h, "gw_jump_passes", (float)passes);
    return CTWS_OK;
}
}  // namespace

extern "C" {

int ctws_graph_components(ctws_handle* h, const uint64_t* edges, int64_t n_edges, const uint64_t* assignments,
                          int64_t n_nodes, uint64_t* out) {
    return graph_components(h, edges, n_edges, assignments, n_nodes, out, false);
}

int ctws_graph_components_device(ctws_handle* h, const uint64_t* edges, int64_t n_edges, const uint64_t* assignments,
                                 int64_t n_nodes, uint64_t* out) {
    return graph_components(h, edges, n_edges, assignments, n_nodes, out, true);
}

int ctws_graph_watershed(ctws_handle* h, const uint64_t* edges, const double* weights, int64_t n_edges,
                         const uint64_t* seeds, int64_t n_nodes, int relabel, uint64_t* out) {
    return graph_watershed(h, edges, weights, n_edges, seeds, n_nodes, relabel, out, false);
}

int ctws_graph_watershed_device(ctws_handle* h, const uint64_t* edges, const double* weights, int64_t n_edges,
                                const uint64_t* seeds, int64_t n_nodes, int relabel, uint64_t* out) {
    return graph_watershed(h, edges, weights, n_edges, seeds, n_nodes, relabel, out, true);
}

}  // extern "C"
