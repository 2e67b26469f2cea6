// ctws_lifted.cpp — host side of libctws.so: LiftedFeaturesFromNodeLabelsWorkflow.
#include "ctws_host.h"

using namespace ctws;

// ---- LiftedFeaturesFromNodeLabelsWorkflow: the sparse lifted neighbourhood (k_lifted.hip) ----
namespace {
// The first capacity of the key buffer depends on the number of labelled nodes alone: 64 keys per
// source (at depth 4 the 128^3 grid of the benchmark emits 19, a block's RAG 43), and never fewer than 2^16.
constexpr int64_t kLfFirstCap = 1 << 16;
constexpr int64_t kLfCapPerSource = 64;
int64_t lf_first_cap(int64_t ns) { return std::max(kLfFirstCap, kLfCapPerSource * ns); }
// Three workgroups of k_lf_bfs share a CU's LDS (54,272 B each); every wave owns a queue and a
// bitmap over the n nodes (4 1/8 bytes per node), and the waves in flight are cut down to what fits
// in this many bytes and in half of the free memory
constexpr int kLfMaxGroups = 256 * 3;
constexpr size_t kLfWaveBudget = (size_t)32 << 30;
// the counter block: the row checks' three words, the sources, and a line for the append counter
enum LfWord : size_t { kLfWordSources = 16, kLfWordEmit = 32, kLfWordVisits = 33, kLfWords = 48 };

int lifted_neighborhood(ctws_handle* h, const uint64_t* edges, int64_t m, const uint64_t* labels, int64_t n, int depth,
                        int mode, uint64_t ignore_label, uint64_t* out, int64_t cap, int64_t* n_out, bool dev) {
    int r;
    if (!h) return CTWS_EINVAL;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    if (n_out) *n_out = 0;
    if (!n_out || m < 0 || n < 0 || cap < 0 || (!out && cap > 0) || (m > 0 && !edges) || (n > 0 && !labels)) {
        h->err = "lifted neighborhood: bad arguments (tables for n_edges > 0 and n_nodes > 0, out for cap > 0)";
        return CTWS_EINVAL;
    }
    if (depth < 1) {
        h->err = "lifted neighborhood: depth " + std::to_string(depth) + " (a lifted edge spans at least 2 hops; depth >= 1)";
        return CTWS_EINVAL;
    }
    if (mode != CTWS_LIFTED_ALL && mode != CTWS_LIFTED_SAME && mode != CTWS_LIFTED_DIFFERENT) {
        h->err = "lifted neighborhood: unknown mode " + std::to_string(mode) + " (0 all, 1 same, 2 different)";
        return CTWS_EINVAL;
    }
    if (n >= (1ll << 32) || m >= (1ll << 31)) {
        h->err = "lifted neighborhood: 2^32 or more nodes or 2^31 or more edges (ids and adjacency offsets are 32-bit)";
        return CTWS_EUNSUPPORTED;
    }
    if (m == 0) return CTWS_OK;  // no edge, no path: no launch
    if (n == 0) {
        h->err = "lifted neighborhood: " + std::to_string(m) + " rows hold an id >= n_nodes (0)";
        return CTWS_EINVAL;
    }
    const uint64_t *de, *dl;
    if ((r = stage_in(h, h->lf_edges, edges, 2 * sizeof(uint64_t) * (size_t)m, dev, &de)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->lf_lab, labels, sizeof(uint64_t) * (size_t)n, dev, &dl)) != CTWS_OK) return r;
    const size_t nb1 = sizeof(uint32_t) * ((size_t)n + 1);
    if ((r = grow(h, h->lf_red, kLfWords * sizeof(uint64_t))) != CTWS_OK) return r;
    if ((r = grow(h, h->lf_deg, nb1)) != CTWS_OK) return r;
    if ((r = grow(h, h->lf_row, nb1)) != CTWS_OK) return r;
    if ((r = grow(h, h->lf_adj, 2 * sizeof(uint32_t) * (size_t)m)) != CTWS_OK) return r;
    if ((r = grow(h, h->lf_src, sizeof(uint32_t) * (size_t)n)) != CTWS_OK) return r;
    unsigned long long* red = (unsigned long long*)h->lf_red.p;
    uint32_t* deg = (uint32_t*)h->lf_deg.p;
    uint32_t* row = (uint32_t*)h->lf_row.p;
    // the rows' checks with the degrees, and the labelled nodes
    HIPCHK(hipMemsetAsync(red, 0, kLfWords * sizeof(uint64_t), h->stream));
    HIPCHK(hipMemsetAsync(deg, 0, nb1, h->stream));
    record(h, 0);
    const unsigned gm = (unsigned)std::min<int64_t>((m + 255) / 256, 8192);
    const unsigned gn = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    k_lf_degrees<<<gm, 256, 0, h->stream>>>(de, (uint32_t)m, (uint64_t)n, deg, red);
    k_lf_sources<<<gn, 256, 0, h->stream>>>(dl, (uint32_t)n, ignore_label, (uint32_t*)h->lf_src.p, red + kLfWordSources);
    LAUNCHCHK();
    unsigned long long w[kLfWordSources + 1];
    HIPCHK(hipMemcpyAsync(w, red, sizeof(w), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (w[kLfBadId] || w[kLfBadUv] || w[kLfBadOrder]) {
        h->err = "lifted neighborhood: the edge table is not a graph's: " + std::to_string(w[kLfBadId]) +
                 " rows hold an id >= n_nodes (" + std::to_string(n) + "), " + std::to_string(w[kLfBadUv]) +
                 " rows have u >= v, " + std::to_string(w[kLfBadOrder]) + " rows are not above their predecessor";
        return CTWS_EINVAL;
    }
    const int64_t ns = (int64_t)w[kLfWordSources];
    if (ns > n) {
        h->err = "lifted neighborhood: the kernel counted " + std::to_string(ns) + " labelled nodes of " + std::to_string(n);
        return CTWS_EHIP;
    }
    add_timing(h, "lf_sources", (float)ns);
    if (ns == 0) return CTWS_OK;  // no labelled node: no search
    // CSR of both directions
    size_t tb_scan = 0;
    HIPCHK(exclusive_sum_u32(nullptr, tb_scan, nullptr, nullptr, n + 1, h->stream));
    if ((r = grow(h, h->prim_tmp, tb_scan)) != CTWS_OK) return r;
    HIPCHK(exclusive_sum_u32(h->prim_tmp.p, tb_scan, deg, row, n + 1, h->stream));
    HIPCHK(hipMemsetAsync(deg, 0, nb1, h->stream));  // (now the fill's cursors)
    k_lf_fill<<<gm, 256, 0, h->stream>>>(de, (uint32_t)m, row, deg, (uint32_t*)h->lf_adj.p);
    LAUNCHCHK();
    record(h, 1);
    // the waves in flight and their queues and bitmaps
    const uint32_t qstride = (uint32_t)std::max<int64_t>(n - kLfQueueLds, 1);
    const uint32_t bstride = (uint32_t)((n + 31) / 32);
    const size_t wave_bytes = sizeof(uint32_t) * ((size_t)qstride + bstride);
    int64_t groups = std::min<int64_t>((ns + kLfWaves - 1) / kLfWaves, kLfMaxGroups);
    size_t free_bytes = 0, total_bytes = 0;
    HIPCHK(hipMemGetInfo(&free_bytes, &total_bytes));
    // (what the handle holds already is its own: a second call takes the waves of the first)
    const size_t budget = std::max(h->lf_queue.bytes + h->lf_bits.bytes, std::min(kLfWaveBudget, free_bytes / 2));
    groups = std::max<int64_t>(1, std::min<int64_t>(groups, (int64_t)(budget / wave_bytes) / kLfWaves));
    const size_t nwaves = (size_t)groups * kLfWaves;
    if ((r = grow(h, h->lf_queue, sizeof(uint32_t) * qstride * nwaves)) != CTWS_OK) return r;
    if ((r = grow(h, h->lf_bits, sizeof(uint32_t) * bstride * nwaves)) != CTWS_OK) return r;
    HIPCHK(hipMemsetAsync(h->lf_bits.p, 0, sizeof(uint32_t) * bstride * nwaves, h->stream));
    int b = 1;  // bits per node id
    while ((1ll << b) < n) ++b;
    LfArgs a;
    a.row = row;
    a.adj = (const uint32_t*)h->lf_adj.p;
    a.lab = dl;
    a.src = (const uint32_t*)h->lf_src.p;
    a.ns = (uint32_t)ns;
    a.depth = (uint32_t)depth;
    a.mode = mode;
    a.ignore = ignore_label;
    a.b = b;
    a.queue = (uint32_t*)h->lf_queue.p;
    a.qstride = qstride;
    a.bits = (uint32_t*)h->lf_bits.p;
    a.bstride = bstride;
    a.count = red + kLfWordEmit;
    a.visits = red + kLfWordVisits;
    EmitCap ecap = {kRedEmit, (unsigned long long)lf_first_cap(ns)};
    Emitted e;
    r = counted_emit(
        h, "lifted neighborhood", red + kLfWordEmit, 2, 2, &ecap, 1,
        [&] {
            const int r = grow(h, h->lf_keys, sizeof(uint64_t) * (size_t)ecap.cap);
            if (r != CTWS_OK) return r;
            a.keys = (uint64_t*)h->lf_keys.p;
            a.cap = ecap.cap;
            k_lf_bfs<<<(unsigned)groups, 64 * kLfWaves, 0, h->stream>>>(a);
            return CTWS_OK;
        },
        [](const unsigned long long*) { return CTWS_OK; }, &e);
    if (r != CTWS_OK) return r;
    record(h, 2);
    const unsigned long long k = e.w[kRedEmit];
    add_timing(h, "lf_bfs_passes", (float)e.passes);
    add_timing(h, "lf_keys", (float)k);
    add_timing(h, "lf_visits", (float)e.w[1]);
    add_timing(h, "lf_waves", (float)nwaves);
    if (k >= (1ull << 31)) {
        h->err = "lifted neighborhood: 2^31 or more lifted edges (" + std::to_string(k) + ") in one call";
        return CTWS_EUNSUPPORTED;
    }
    *n_out = (int64_t)k;
    if ((int64_t)k > cap) {
        h->err = "lifted neighborhood: output capacity too small";
        return CTWS_EINVAL;
    }
    if (k == 0) {
        HIPCHK(hipStreamSynchronize(h->stream));
        return CTWS_OK;
    }
    uint64_t* dout;
    const size_t out_bytes = 2 * sizeof(uint64_t) * (size_t)k;
    if ((r = out_begin(h, h->lf_out, out, out_bytes, dev, &dout)) != CTWS_OK) return r;
    size_t tb_sort = 0;
    HIPCHK(sort_keys_u64(nullptr, tb_sort, nullptr, nullptr, (int64_t)k, 2 * b, h->stream));
    if ((r = grow(h, h->lf_skeys, sizeof(uint64_t) * (size_t)k)) != CTWS_OK) return r;
    if ((r = grow(h, h->prim_tmp, tb_sort)) != CTWS_OK) return r;
    HIPCHK(sort_keys_u64(h->prim_tmp.p, tb_sort, (const uint64_t*)h->lf_keys.p, (uint64_t*)h->lf_skeys.p,
                         (int64_t)k, 2 * b, h->stream));
    const unsigned gk = (unsigned)std::min<int64_t>(((int64_t)k + 255) / 256, 8192);
    k_lf_unpack<<<gk, 256, 0, h->stream>>>((const uint64_t*)h->lf_skeys.p, (int64_t)k, b, dout);
    LAUNCHCHK();
    record(h, 3);
    if ((r = out_end(h, out, dout, out_bytes, dev)) != CTWS_OK) return r;
    stage_time(h, "lf_csr", 0, 1);
    stage_time(h, "lf_bfs", 1, 2);
    stage_time(h, "lf_sort", 2, 3);
    return CTWS_OK;
}
}  // namespace

extern "C" {

int ctws_lifted_neighborhood(ctws_handle* h, const uint64_t* edges, int64_t n_edges, const uint64_t* node_labels,
                             int64_t n_nodes, int depth, int mode, uint64_t ignore_label, uint64_t* out, int64_t cap,
                             int64_t* n_out) {
    return lifted_neighborhood(h, edges, n_edges, node_labels, n_nodes, depth, mode, ignore_label, out, cap, n_out,
                               false);
}

int ctws_lifted_neighborhood_device(ctws_handle* h, const uint64_t* edges, int64_t n_edges,
                                    const uint64_t* node_labels, int64_t n_nodes, int depth, int mode,
                                    uint64_t ignore_label, uint64_t* out, int64_t cap, int64_t* n_out) {
    return lifted_neighborhood(h, edges, n_edges, node_labels, n_nodes, depth, mode, ignore_label, out, cap, n_out,
                               true);
}

int ctws_lifted_limits(int64_t n_sources, int64_t* first_capacity, int64_t* visited_capacity) {
    if (n_sources < 0) return CTWS_EINVAL;
    if (first_capacity) *first_capacity = lf_first_cap(n_sources);
    if (visited_capacity) *visited_capacity = kLfHashFill;
    return CTWS_OK;
}

}  // extern "C"
