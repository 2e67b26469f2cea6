// ctws_graph.cpp — host side of libctws.so: the features that live on the graph path's buffers (rg_*)
// and on sort_by_id: the region adjacency graph and unique pairs, label overlaps, morphology,
// region features, and the edge features (which use the graph's key kernels).
#include "ctws_host.h"

using namespace ctws;

// ---- GraphWorkflow: the region adjacency graph (k_rag.hip) ----------------------------------
namespace {
// The sorted distinct values of dv (device) into rg_tab, by the relabel path's radix sort and
// run-length encoding: these are id tables with many repeats of few values over a narrow range,
// where the bitmap unique's atomics all land in a few words (57 ms for the 16.8 M labels of a
// block of fragments, measured).  The table grows to the size the first call reports.
int rag_table(ctws_handle* h, const uint64_t* dv, int64_t n, int64_t* nt) {
    int r;
    *nt = 0;
    if (n == 0) return CTWS_OK;
    const int64_t cap = std::max<int64_t>((int64_t)(h->rg_tab.bytes / sizeof(uint64_t)), 1 << 16);
    if ((r = grow(h, h->rg_tab, sizeof(uint64_t) * (size_t)cap)) != CTWS_OK) return r;
    r = unique_sorted(h, dv, n, 1, (uint64_t*)h->rg_tab.p, nullptr, cap, nt);
    if (r == CTWS_EINVAL && *nt > cap) {
        const int64_t want = *nt;
        h->err.clear();
        if ((r = grow(h, h->rg_tab, sizeof(uint64_t) * (size_t)want)) != CTWS_OK) return r;
        r = unique_sorted(h, dv, n, 1, (uint64_t*)h->rg_tab.p, nullptr, want, nt);
    }
    return r;
}

// The tail both entry points share: n (pair, weight) records on the device -> the sorted unique
// pairs in rg_out (m x 2) with their summed weights in rg_sum (m).  tab (device, ascending)
// holds every endpoint value; weights == nullptr counts 1 per record.
int pairs_tail(ctws_handle* h, const uint64_t* pairs, const uint64_t* weights, int64_t n, const uint64_t* tab,
               int64_t nt, int64_t* m) {
    *m = 0;
    if (n == 0) return CTWS_OK;
    if (n >= (1ll << 31)) {
        h->err = "unique pairs: more than 2^31 - 1 pairs in one call";
        return CTWS_EUNSUPPORTED;
    }
    if (nt >= (1ll << 32)) {
        h->err = "unique pairs: 2^32 or more distinct ids in one call (the sort keys hold two 32-bit ranks)";
        return CTWS_EUNSUPPORTED;
    }
    int b = 1;  // bits per rank
    while ((1ll << b) < nt) ++b;
    int r;
    const size_t nb = sizeof(uint64_t) * (size_t)n;
    size_t tb_sort = 0, tb_red = 0;
    HIPCHK(sort_pairs_u64(nullptr, tb_sort, nullptr, nullptr, nullptr, nullptr, n, 2 * b, h->stream));
    HIPCHK(reduce_by_key_sum_u64(nullptr, tb_red, nullptr, nullptr, nullptr, nullptr, nullptr, n, h->stream));
    if ((r = grow(h, h->rg_keys, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_skeys, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_sw, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_sum, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->prim_tmp, std::max(tb_sort, tb_red))) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_red, kRedWords * sizeof(uint64_t))) != CTWS_OK) return r;
    if (!weights && (r = grow(h, h->rg_w, nb)) != CTWS_OK) return r;
    uint64_t* keys = (uint64_t*)h->rg_keys.p;
    uint64_t* skeys = (uint64_t*)h->rg_skeys.p;
    uint64_t* sw = (uint64_t*)h->rg_sw.p;
    uint64_t* sums = (uint64_t*)h->rg_sum.p;
    unsigned long long* red = (unsigned long long*)h->rg_red.p;
    const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    HIPCHK(hipMemsetAsync(red + kRedPairRuns, 0, 2 * sizeof(uint64_t), h->stream));  // (and kRedPairMiss)
    record(h, 2);
    if (!weights) {
        k_pair_ones<<<g, 256, 0, h->stream>>>((uint64_t*)h->rg_w.p, n);
        weights = (const uint64_t*)h->rg_w.p;
    }
    k_pair_keys<<<g, 256, 0, h->stream>>>(pairs, n, tab, nt, b, keys, red + kRedPairMiss);
    LAUNCHCHK();
    record(h, 3);
    HIPCHK(sort_pairs_u64(h->prim_tmp.p, tb_sort, keys, skeys, weights, sw, n, 2 * b, h->stream));
    record(h, 4);
    // (the unsorted keys are dead: their buffer takes the unique keys)
    HIPCHK(reduce_by_key_sum_u64(h->prim_tmp.p, tb_red, skeys, keys, sw, sums, (uint64_t*)(red + kRedPairRuns),
                                 n, h->stream));
    record(h, 5);
    unsigned long long hr[2] = {0ull, 0ull};
    HIPCHK(hipMemcpyAsync(hr, red + kRedPairRuns, sizeof(hr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (hr[1]) {
        h->err = "unique pairs: " + std::to_string(hr[1]) + " endpoint values are missing from the id table";
        return CTWS_EINVAL;
    }
    *m = (int64_t)hr[0];
    if ((r = grow(h, h->rg_out, 2 * sizeof(uint64_t) * (size_t)*m)) != CTWS_OK) return r;
    const unsigned gm = (unsigned)std::min<int64_t>((*m + 255) / 256, 8192);
    k_pair_unpack<<<gm, 256, 0, h->stream>>>(keys, *m, tab, b, (uint64_t*)h->rg_out.p);
    LAUNCHCHK();
    record(h, 6);
    HIPCHK(hipStreamSynchronize(h->stream));
    stage_time(h, "pair_keys", 2, 3);
    stage_time(h, "pair_sort", 3, 4);
    stage_time(h, "pair_reduce", 4, 5);
    stage_time(h, "pair_unpack", 5, 6);
    return CTWS_OK;
}

// the tail's result -> the caller's buffers (the sizes are known to fit)
int pairs_out(ctws_handle* h, int64_t m, int on_device, uint64_t* out, uint64_t* counts) {
    if (m) {
        const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        HIPCHK(hipMemcpyAsync(out, h->rg_out.p, 2 * sizeof(uint64_t) * (size_t)m, k, h->stream));
        if (counts) HIPCHK(hipMemcpyAsync(counts, h->rg_sum.p, sizeof(uint64_t) * (size_t)m, k, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTWS_OK;
}

int rag_block(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx, int ignore_label,
              uint64_t* nodes, int64_t cap_nodes, int64_t* n_nodes, uint64_t* edges, uint64_t* counts,
              int64_t cap_edges, int64_t* n_edges, bool dev) {
    if (!h || !labels || nz <= 0 || ny <= 0 || nx <= 0 || !n_nodes || !n_edges || cap_nodes < 0 || cap_edges < 0 ||
        (!nodes && cap_nodes > 0) || (!edges && cap_edges > 0))
        return CTWS_EINVAL;
    int r;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    *n_nodes = *n_edges = 0;
    r = check_extent(h, nz, ny, nx, "rag block", "block", "the pair kernel indexes a block with 32 bits");
    if (r != CTWS_OK) return r;
    const int64_t N = nz * ny * nx;
    const uint64_t* dl;
    if ((r = stage_in(h, h->rg_lab, labels, sizeof(uint64_t) * (size_t)N, dev, &dl)) != CTWS_OK) return r;
    // one pass emits the pairs and the node ids, into first buffers of a quarter / a sixteenth of
    // the voxels
    if ((r = grow(h, h->rg_red, kRedWords * sizeof(uint64_t))) != CTWS_OK) return r;
    unsigned long long* cnt = (unsigned long long*)h->rg_red.p;
    RagArgs a;
    a.lab = dl;
    a.nz = (uint32_t)nz;
    a.ny = (uint32_t)ny;
    a.nx = (uint32_t)nx;
    a.ignore = ignore_label ? 1 : 0;
    a.count = cnt;
    a.ncount = cnt + kRedNodes;
    const int64_t rows = nz * ny;
    // four workgroups per CU (their LDS stages) and no more: every wave ends with an append of
    // its own, and one counter word takes only ~85 returning atomics per microsecond
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, 1024));
    EmitCap caps[2] = {{kRedEmit, first_cap(N, 4)}, {kRedNodes, first_cap(N, 16)}};
    Emitted e;
    record(h, 0);
    r = counted_emit(
        h, "rag block", cnt, kRedNodes + 1, kRedNodes + 1, caps, 2,
        [&] {
            int r;
            if ((r = grow(h, h->rg_pairs, 2 * sizeof(uint64_t) * (size_t)caps[0].cap)) != CTWS_OK) return r;
            if ((r = grow(h, h->rg_w, sizeof(uint64_t) * (size_t)caps[0].cap)) != CTWS_OK) return r;
            if ((r = grow(h, h->rg_nodes, sizeof(uint64_t) * (size_t)caps[1].cap)) != CTWS_OK) return r;
            a.pairs = (uint64_t*)h->rg_pairs.p;
            a.weights = (uint64_t*)h->rg_w.p;
            a.nodes = (uint64_t*)h->rg_nodes.p;
            a.cap = caps[0].cap;
            a.ncap = caps[1].cap;
            k_rag_pairs<<<g, 256, 0, h->stream>>>(a);
            return CTWS_OK;
        },
        [](const unsigned long long*) { return CTWS_OK; }, &e);
    if (r != CTWS_OK) return r;
    const int64_t n_pairs = (int64_t)e.w[kRedEmit], n_ids = (int64_t)e.w[kRedNodes];
    record(h, 1);
    // nodes: the sorted unique of the emitted ids = np.unique of the block (without 0 under
    // ignore_label: the kernel emits no 0 then)
    int64_t nt = 0;
    if ((r = rag_table(h, (const uint64_t*)h->rg_nodes.p, n_ids, &nt)) != CTWS_OK) return r;
    const uint64_t* tab = (const uint64_t*)h->rg_tab.p;
    record(h, 7);
    HIPCHK(hipStreamSynchronize(h->stream));
    stage_time(h, "rag_pairs", 0, 1);
    stage_time(h, "rag_nodes", 1, 7);
    add_timing(h, "rag_pair_passes", (float)e.passes);  // (counts, as the flood's rounds)
    add_timing(h, "rag_emits", (float)n_pairs);
    add_timing(h, "rag_node_emits", (float)n_ids);
    int64_t m = 0;
    if ((r = pairs_tail(h, (const uint64_t*)h->rg_pairs.p, (const uint64_t*)h->rg_w.p, n_pairs, tab, nt, &m)) !=
        CTWS_OK)
        return r;
    *n_nodes = nt;
    *n_edges = m;
    if (*n_nodes > cap_nodes || m > cap_edges) {
        h->err = "rag block: output capacity too small";
        return CTWS_EINVAL;
    }
    if (*n_nodes)
        HIPCHK(hipMemcpyAsync(nodes, tab, sizeof(uint64_t) * (size_t)*n_nodes,
                              dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    return pairs_out(h, m, dev ? 1 : 0, edges, counts);
}
}  // namespace

extern "C" {

int ctws_unique_pairs_u64(ctws_handle* h, const uint64_t* pairs, const uint64_t* weights, int64_t n, int on_device,
                          uint64_t* out, uint64_t* counts, int64_t cap, int64_t* n_unique) {
    if (!h || (!pairs && n > 0) || n < 0 || !n_unique || cap < 0 || (!out && cap > 0)) return CTWS_EINVAL;
    int r;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    *n_unique = 0;
    if (n == 0) return CTWS_OK;
    if (n >= (1ll << 30)) {
        h->err = "unique pairs: 2^30 or more pairs in one call";
        return CTWS_EUNSUPPORTED;
    }
    const bool dev = on_device != 0;
    if ((r = stage_in(h, h->rg_pairs, pairs, 2 * sizeof(uint64_t) * (size_t)n, dev, &pairs)) != CTWS_OK) return r;
    if (weights && (r = stage_in(h, h->rg_lab, weights, sizeof(uint64_t) * (size_t)n, dev, &weights)) != CTWS_OK)
        return r;
    // ids -> ranks: the distinct endpoint values
    int64_t nt = 0;
    if ((r = rag_table(h, pairs, 2 * n, &nt)) != CTWS_OK) return r;
    int64_t m = 0;
    if ((r = pairs_tail(h, pairs, weights, n, (const uint64_t*)h->rg_tab.p, nt, &m)) != CTWS_OK) return r;
    *n_unique = m;
    if (m > cap) {
        h->err = "ctws_unique_pairs_u64: output capacity too small";
        return CTWS_EINVAL;
    }
    return pairs_out(h, m, on_device, out, counts);
}

int ctws_rag_block(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx, int ignore_label,
                   uint64_t* nodes, int64_t cap_nodes, int64_t* n_nodes, uint64_t* edges, uint64_t* counts,
                   int64_t cap_edges, int64_t* n_edges) {
    return rag_block(h, labels, nz, ny, nx, ignore_label, nodes, cap_nodes, n_nodes, edges, counts, cap_edges, n_edges,
                     false);
}

int ctws_rag_block_device(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx, int ignore_label,
                          uint64_t* nodes, int64_t cap_nodes, int64_t* n_nodes, uint64_t* edges, uint64_t* counts,
                          int64_t cap_edges, int64_t* n_edges) {
    return rag_block(h, labels, nz, ny, nx, ignore_label, nodes, cap_nodes, n_nodes, edges, counts, cap_edges, n_edges,
                     true);
}

}  // extern "C"

// ---- NodeLabelWorkflow: fragment / label overlaps (k_overlaps.hip) ---------------------------
namespace {
int label_overlaps(ctws_handle* h, const uint64_t* nodes_vol, const uint64_t* labels_vol, int64_t n, int with_ignore,
                   uint64_t ignore_label, uint64_t* rows, int64_t cap, int64_t* n_rows, bool dev) {
    if (!h || n < 0 || ((!nodes_vol || !labels_vol) && n > 0) || !n_rows || cap < 0 || (!rows && cap > 0))
        return CTWS_EINVAL;
    int r;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    *n_rows = 0;
    if (n == 0) return CTWS_OK;
    r = check_extent(h, 1, 1, n, "label overlaps", "call", "the pair kernel indexes the arrays with 32 bits");
    if (r != CTWS_OK) return r;
    const size_t nb = sizeof(uint64_t) * (size_t)n;
    const uint64_t *dn, *dl;
    if ((r = stage_in(h, h->rg_lab, nodes_vol, nb, dev, &dn)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->ov_lab, labels_vol, nb, dev, &dl)) != CTWS_OK) return r;
    // the run heads, at most one per voxel, into a first buffer of a quarter of the voxels
    if ((r = grow(h, h->rg_red, kRedWords * sizeof(uint64_t))) != CTWS_OK) return r;
    unsigned long long* cnt = (unsigned long long*)h->rg_red.p;
    OvArgs a;
    a.nodes = dn;
    a.labels = dl;
    a.n = (uint32_t)n;
    a.with_ignore = with_ignore ? 1 : 0;
    a.ignore_label = ignore_label;
    a.count = cnt;
    const int64_t words = (n + 63) / 64;
    // four workgroups per CU, as k_rag_pairs: every wave ends with an append of its own
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((words + 3) / 4, 1024));
    EmitCap ecap = {kRedEmit, first_cap(n, 4)};
    Emitted e;
    record(h, 0);
    r = counted_emit(
        h, "label overlaps", cnt, 1, 1, &ecap, 1,
        [&] {
            int r;
            if ((r = grow(h, h->rg_pairs, 2 * sizeof(uint64_t) * (size_t)ecap.cap)) != CTWS_OK) return r;
            if ((r = grow(h, h->rg_w, sizeof(uint64_t) * (size_t)ecap.cap)) != CTWS_OK) return r;
            a.pairs = (uint64_t*)h->rg_pairs.p;
            a.weights = (uint64_t*)h->rg_w.p;
            a.cap = ecap.cap;
            k_ov_pairs<<<g, 256, 0, h->stream>>>(a);
            return CTWS_OK;
        },
        [&](const unsigned long long* w) { return runs_within(h, "label overlaps", w[kRedEmit], 0, n); }, &e);
    if (r != CTWS_OK) return r;
    const unsigned long long emitted = e.w[kRedEmit];
    record(h, 1);
    HIPCHK(hipStreamSynchronize(h->stream));
    stage_time(h, "ov_pairs", 0, 1);
    add_timing(h, "ov_pair_passes", (float)e.passes);  // (counts, as the flood's rounds)
    add_timing(h, "ov_emits", (float)emitted);
    if (emitted == 0) return CTWS_OK;  // every voxel carries the ignore label
    if (emitted >= (1ull << 30)) {
        h->err = "label overlaps: 2^30 or more runs of equal (node, label) pairs in one call";
        return CTWS_EUNSUPPORTED;
    }
    // ids -> ranks in one table for both sides: the key order is the (node, label) order
    int64_t nt = 0, m = 0;
    if ((r = rag_table(h, (const uint64_t*)h->rg_pairs.p, 2 * (int64_t)emitted, &nt)) != CTWS_OK) return r;
    record(h, 7);
    HIPCHK(hipStreamSynchronize(h->stream));
    stage_time(h, "ov_table", 1, 7);
    if ((r = pairs_tail(h, (const uint64_t*)h->rg_pairs.p, (const uint64_t*)h->rg_w.p, (int64_t)emitted,
                        (const uint64_t*)h->rg_tab.p, nt, &m)) != CTWS_OK)
        return r;
    *n_rows = m;
    if (m > cap) {
        h->err = "label overlaps: output capacity too small";
        return CTWS_EINVAL;
    }
    const size_t rb = 3 * sizeof(uint64_t) * (size_t)m;
    uint64_t* drows;
    if ((r = out_begin(h, h->ov_rows, rows, rb, dev, &drows)) != CTWS_OK) return r;
    const unsigned gm = (unsigned)std::min<int64_t>((m + 255) / 256, 8192);
    k_ov_rows<<<gm, 256, 0, h->stream>>>((const uint64_t*)h->rg_out.p, (const uint64_t*)h->rg_sum.p, m, drows);
    LAUNCHCHK();
    return out_end(h, rows, drows, rb, dev);
}
}  // namespace

extern "C" {

int ctws_label_overlaps(ctws_handle* h, const uint64_t* nodes_vol, const uint64_t* labels_vol, int64_t n,
                        int with_ignore, uint64_t ignore_label, uint64_t* rows, int64_t cap, int64_t* n_rows) {
    return label_overlaps(h, nodes_vol, labels_vol, n, with_ignore, ignore_label, rows, cap, n_rows, false);
}

int ctws_label_overlaps_device(ctws_handle* h, const uint64_t* nodes_vol, const uint64_t* labels_vol, int64_t n,
                               int with_ignore, uint64_t ignore_label, uint64_t* rows, int64_t cap, int64_t* n_rows) {
    return label_overlaps(h, nodes_vol, labels_vol, n, with_ignore, ignore_label, rows, cap, n_rows, true);
}

}  // extern "C"

// ---- MorphologyWorkflow: size, centre and bounding box per id (k_morph.hip) ------------------
namespace {
int block_morphology(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx, const int64_t* begin,
                     double* rows, int64_t cap, int64_t* n_rows, bool dev) {
    if (!h || !labels || nz <= 0 || ny <= 0 || nx <= 0 || !begin || !n_rows || cap < 0 || (!rows && cap > 0))
        return CTWS_EINVAL;
    int r;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    *n_rows = 0;
    if (begin[0] < 0 || begin[1] < 0 || begin[2] < 0) {
        h->err = "block morphology: a negative begin";
        return CTWS_EINVAL;
    }
    // the record packs z, y, x0 into 19 bits each; begin + extent <= 2^21 and fewer than 2^31
    // voxels keep every coordinate sum below 2^52, exact in a double
    constexpr int64_t kExt = 1ll << 19, kCoord = 1ll << 21;
    if (nz >= kExt || ny >= kExt || nx >= kExt) {
        h->err = "block morphology: an extent of 2^19 or more (the run record holds 19 bits per coordinate)";
        return CTWS_EUNSUPPORTED;
    }
    r = check_extent(h, nz, ny, nx, "block morphology", "block", "the run kernel indexes a block with 32 bits");
    if (r != CTWS_OK) return r;
    const int64_t ext[3] = {nz, ny, nx};
    for (int d = 0; d < 3; ++d)
        if (begin[d] > kCoord || begin[d] + ext[d] > kCoord) {
            h->err = "block morphology: begin + extent above 2^21 (the coordinate sums would not be exact doubles)";
            return CTWS_EUNSUPPORTED;
        }
    const int64_t N = nz * ny * nx;
    const uint64_t* dl;
    if ((r = stage_in(h, h->rg_lab, labels, sizeof(uint64_t) * (size_t)N, dev, &dl)) != CTWS_OK) return r;
    // the run heads, at least one and at most one per voxel, into a first buffer of a quarter of
    // the voxels
    if ((r = grow(h, h->rg_red, kRedWords * sizeof(uint64_t))) != CTWS_OK) return r;
    unsigned long long* cnt = (unsigned long long*)h->rg_red.p;
    MorphArgs a;
    a.lab = dl;
    a.nz = (uint32_t)nz;
    a.ny = (uint32_t)ny;
    a.nx = (uint32_t)nx;
    a.count = cnt;
    a.vmax = cnt + kRedVmax;
    const int64_t lines = nz * ny;
    // four workgroups per CU, as k_rag_pairs: every wave ends with an append of its own
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((lines + 3) / 4, 1024));
    EmitCap ecap = {kRedEmit, first_cap(N, 4)};
    Emitted e;
    record(h, 0);
    r = counted_emit(
        h, "block morphology", cnt, kRedVmax + 1, kRedVmax + 1, &ecap, 1,
        [&] {
            int r;
            if ((r = grow(h, h->rg_pairs, sizeof(uint64_t) * (size_t)ecap.cap)) != CTWS_OK) return r;
            if ((r = grow(h, h->rg_w, sizeof(uint64_t) * (size_t)ecap.cap)) != CTWS_OK) return r;
            a.ids = (uint64_t*)h->rg_pairs.p;
            a.recs = (uint64_t*)h->rg_w.p;
            a.cap = ecap.cap;
            k_morph_runs<<<g, 256, 0, h->stream>>>(a);
            return CTWS_OK;
        },
        [&](const unsigned long long* w) { return runs_within(h, "block morphology", w[kRedEmit], 1, N); }, &e);
    if (r != CTWS_OK) return r;
    const int64_t n = (int64_t)e.w[kRedEmit];  // (< 2^31)
    record(h, 1);
    // the largest id was taken by the run pass
    ById s;
    if ((r = sort_by_id(h, "block morphology", a.ids, a.recs, n, e.w[kRedVmax], 2, &s)) != CTWS_OK) return r;
    stage_time(h, "morph_runs", 0, 1);
    stage_time(h, "morph_sort", 1, 2);
    add_timing(h, "morph_run_passes", (float)e.passes);  // (counts, as the flood's rounds)
    add_timing(h, "morph_emits", (float)n);
    const int64_t m = s.m;
    *n_rows = m;
    if (m > cap) {
        h->err = "block morphology: output capacity too small";
        return CTWS_EINVAL;
    }
    const size_t rb = 11 * sizeof(double) * (size_t)m;
    double* drows;
    if ((r = out_begin(h, h->mo_rows, rows, rb, dev, &drows)) != CTWS_OK) return r;
    // the per-id table of the split segments: ten integers per id, zero = neutral
    const size_t ab = 10 * sizeof(uint64_t) * (size_t)m;
    if ((r = grow(h, h->mo_acc, ab)) != CTWS_OK) return r;
    unsigned long long* acc = (unsigned long long*)h->mo_acc.p;
    HIPCHK(hipMemsetAsync(acc, 0, ab, h->stream));
    const MorphBegin b = {(uint64_t)begin[0], (uint64_t)begin[1], (uint64_t)begin[2]};
    const int64_t waves = m + n / kMorphChunk;  // a wave per id and per whole chunk of records
    const unsigned gm = (unsigned)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, 2048));
    k_morph_rows<<<gm, 256, 0, h->stream>>>(s.sids, s.srecs, (uint32_t)n, s.uniq, s.counts, (uint32_t)m, b, acc, drows);
    LAUNCHCHK();
    if (n >= (int64_t)kMorphChunk) {  // (a shorter record list holds no whole chunk: no split segment)
        const unsigned gl = (unsigned)std::min<int64_t>((m + 255) / 256, 1024);
        k_morph_long_rows<<<gl, 256, 0, h->stream>>>(s.uniq, (uint32_t)m, b, acc, drows);
        LAUNCHCHK();
    }
    record(h, 3);
    if ((r = out_end(h, rows, drows, rb, dev)) != CTWS_OK) return r;
    stage_time(h, "morph_rows", 2, 3);
    return CTWS_OK;
}
}  // namespace

extern "C" {

int ctws_block_morphology(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx,
                          const int64_t begin[3], double* rows, int64_t cap, int64_t* n_rows) {
    return block_morphology(h, labels, nz, ny, nx, begin, rows, cap, n_rows, false);
}

int ctws_block_morphology_device(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx,
                                 const int64_t begin[3], double* rows, int64_t cap, int64_t* n_rows) {
    return block_morphology(h, labels, nz, ny, nx, begin, rows, cap, n_rows, true);
}

}  // extern "C"

// ---- RegionFeaturesWorkflow: count and mean input value per id (k_regfeat.hip) --------------
namespace {
int region_features_block(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype, int64_t nz,
                          int64_t ny, int64_t nx, int with_ignore, uint64_t ignore_label, double* rows, int64_t cap,
                          int64_t* n_rows, bool dev) {
    if (!h || !labels || !data || nz <= 0 || ny <= 0 || nx <= 0 || !n_rows || cap < 0 || (!rows && cap > 0))
        return CTWS_EINVAL;
    int r;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    *n_rows = 0;
    if (data_dtype != CTWS_U8 && data_dtype != CTWS_U16 && data_dtype != CTWS_F32 && data_dtype != CTWS_F64) {
        h->err = "region features: the input map is uint8, uint16, float32 or float64";
        return CTWS_EINVAL;
    }
    r = check_extent(h, nz, ny, nx, "region features", "block", "the kernels index a block with 32 bits");
    if (r != CTWS_OK) return r;
    const int64_t N = nz * ny * nx, lines = nz * ny;
    if (lines + 1 >= (1ll << 31)) {  // (the scan takes the rows' counts and one 0 behind them with a 32-bit size)
        h->err = "region features: 2^31 - 1 rows in one block (the scan of the rows' run counts is 32-bit)";
        return CTWS_EUNSUPPORTED;
    }
    const size_t es = data_dtype == CTWS_U8 ? 1 : data_dtype == CTWS_U16 ? 2 : data_dtype == CTWS_F32 ? 4 : 8;
    const uint64_t* dl;
    const void* dd;
    if ((r = stage_in(h, h->rg_lab, labels, sizeof(uint64_t) * (size_t)N, dev, &dl)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->rf_data, data, es * (size_t)N, dev, &dd)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_red, kRedWords * sizeof(uint64_t))) != CTWS_OK) return r;
    unsigned long long* red = (unsigned long long*)h->rg_red.p;
    // the rows' run counts with one 0 behind them: the scan's last entry is the total
    const size_t cb = sizeof(uint32_t) * (size_t)(lines + 1);
    size_t tb_scan = 0;
    HIPCHK(exclusive_sum_u32(nullptr, tb_scan, nullptr, nullptr, lines + 1, h->stream));
    if ((r = grow(h, h->rf_cnt, cb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rf_off, cb)) != CTWS_OK) return r;
    if ((r = grow(h, h->prim_tmp, tb_scan)) != CTWS_OK) return r;
    uint32_t* rcnt = (uint32_t*)h->rf_cnt.p;
    uint32_t* roff = (uint32_t*)h->rf_off.p;
    // four workgroups per CU, a wave per row
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((lines + 3) / 4, 1024));
    record(h, 0);
    HIPCHK(hipMemsetAsync(rcnt + lines, 0, sizeof(uint32_t), h->stream));
    HIPCHK(hipMemsetAsync(red, 0, kRedWords * sizeof(uint64_t), h->stream));
    k_regfeat_count<<<g, 256, 0, h->stream>>>(dl, (uint32_t)lines, (uint32_t)nx, rcnt);
    LAUNCHCHK();
    HIPCHK(exclusive_sum_u32(h->prim_tmp.p, tb_scan, rcnt, roff, lines + 1, h->stream));
    record(h, 1);
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, roff + lines, sizeof(total), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (total == 0 || (int64_t)total > N) {
        h->err = "region features: the count kernel found " + std::to_string(total) + " runs";
        return CTWS_EHIP;
    }
    const int64_t n = (int64_t)total;  // (< 2^31): the record arrays hold exactly the runs
    const size_t nb = sizeof(uint64_t) * (size_t)n;
    if ((r = grow(h, h->rg_pairs, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_w, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rf_sums, sizeof(double) * (size_t)n)) != CTWS_OK) return r;
    RegfeatArgs a;
    a.lab = dl;
    a.data = dd;
    a.rows = (uint32_t)lines;
    a.nx = (uint32_t)nx;
    a.with_ignore = with_ignore ? 1 : 0;
    a.ignore = ignore_label;
    a.row_first = roff;
    a.n = total;
    a.ids = (uint64_t*)h->rg_pairs.p;
    a.vals = (uint64_t*)h->rg_w.p;
    a.sums = (double*)h->rf_sums.p;
    a.vmax = red + kRedVmax;
    if (data_dtype == CTWS_U8) k_regfeat_runs<uint8_t><<<g, 256, 0, h->stream>>>(a);
    else if (data_dtype == CTWS_U16) k_regfeat_runs<uint16_t><<<g, 256, 0, h->stream>>>(a);
    else if (data_dtype == CTWS_F32) k_regfeat_runs<float><<<g, 256, 0, h->stream>>>(a);
    else k_regfeat_runs<double><<<g, 256, 0, h->stream>>>(a);
    LAUNCHCHK();
    record(h, 2);
    unsigned long long vmax = 0;  // the largest id
    HIPCHK(hipMemcpyAsync(&vmax, red + kRedVmax, sizeof(vmax), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    ById s;
    if ((r = sort_by_id(h, "region features", a.ids, a.vals, n, vmax, 3, &s)) != CTWS_OK) return r;
    stage_time(h, "regfeat_count", 0, 1);
    stage_time(h, "regfeat_runs", 1, 2);
    stage_time(h, "regfeat_sort", 2, 3);
    add_timing(h, "regfeat_records", (float)total);  // (a count, as the flood's rounds)
    const int64_t m = s.m;
    *n_rows = m;
    if (m > cap) {
        h->err = "region features: output capacity too small";
        return CTWS_EINVAL;
    }
    const size_t rb = 3 * sizeof(double) * (size_t)m;
    double* drows;
    if ((r = out_begin(h, h->rf_rows, rows, rb, dev, &drows)) != CTWS_OK) return r;
    // the chunk table: (n, sum) per whole aligned chunk of sorted records, the n first
    const int64_t chunks = n / kRegfeatChunk;
    if ((r = grow(h, h->rf_ctab, 2 * sizeof(uint64_t) * (size_t)std::max<int64_t>(1, chunks))) != CTWS_OK) return r;
    uint64_t* chunk_n = (uint64_t*)h->rf_ctab.p;
    double* chunk_s = (double*)(chunk_n + std::max<int64_t>(1, chunks));
    if (chunks > 0) {
        const unsigned gc = (unsigned)std::min<int64_t>((chunks + 3) / 4, 2048);
        k_regfeat_chunks<<<gc, 256, 0, h->stream>>>(s.sids, s.srecs, a.sums, total, chunk_n, chunk_s);
        LAUNCHCHK();
    }
    const unsigned gm = (unsigned)std::max<int64_t>(1, std::min<int64_t>((m + 3) / 4, 2048));
    k_regfeat_rows<<<gm, 256, 0, h->stream>>>(s.sids, s.srecs, a.sums, total, s.uniq, s.counts, (uint32_t)m, chunk_n,
                                              chunk_s, drows);
    LAUNCHCHK();
    record(h, 4);
    if ((r = out_end(h, rows, drows, rb, dev)) != CTWS_OK) return r;
    stage_time(h, "regfeat_rows", 3, 4);
    return CTWS_OK;
}
}  // namespace

extern "C" {

int ctws_region_features_block(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype, int64_t nz,
                               int64_t ny, int64_t nx, int with_ignore, uint64_t ignore_label, double* rows,
                               int64_t cap, int64_t* n_rows) {
    return region_features_block(h, labels, data, data_dtype, nz, ny, nx, with_ignore, ignore_label, rows, cap,
                                 n_rows, false);
}

int ctws_region_features_block_device(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype,
                                      int64_t nz, int64_t ny, int64_t nx, int with_ignore, uint64_t ignore_label,
                                      double* rows, int64_t cap, int64_t* n_rows) {
    return region_features_block(h, labels, data, data_dtype, nz, ny, nx, with_ignore, ignore_label, rows, cap,
                                 n_rows, true);
}

}  // extern "C"

// ---- EdgeFeaturesWorkflow: boundary-map statistics per edge (k_edgefeat.hip) ----------------
namespace {
int edge_features_block(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype, int64_t nz,
                        int64_t ny, int64_t nx, int64_t cz, int64_t cy, int64_t cx, int ignore_label,
                        const uint64_t* nodes, int64_t n_nodes, const uint64_t* edges, int64_t n_edges, double* out,
                        int64_t* n_missing, bool dev) {
    int r;
    if (!h) return CTWS_EINVAL;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    if (n_missing) *n_missing = 0;
    if (!labels || !data || nz <= 0 || ny <= 0 || nx <= 0 || cz <= 0 || cy <= 0 || cx <= 0 || cz > nz || cy > ny ||
        cx > nx || n_nodes < 0 || n_edges < 0 || (n_edges > 0 && (!nodes || !edges || !out || n_nodes == 0))) {
        h->err = "edge features: bad arguments (3-D boxes with 0 < core <= extended, tables for n_edges > 0)";
        return CTWS_EINVAL;
    }
    if (data_dtype != CTWS_F32 && data_dtype != CTWS_U8) {
        h->err = "edge features: the boundary map is float32 or uint8";
        return CTWS_EUNSUPPORTED;
    }
    if (n_edges == 0) return CTWS_OK;  // nothing to accumulate into: no launch
    r = check_extent(h, nz, ny, nx, "edge features", "block", "the sample kernel indexes a block with 32 bits");
    if (r != CTWS_OK) return r;
    if (n_nodes >= (1ll << 32) || n_edges >= (1ll << 32)) {
        h->err = "edge features: 2^32 or more nodes or edges in one block";
        return CTWS_EUNSUPPORTED;
    }
    const int64_t N = nz * ny * nx;
    const size_t es = data_dtype == CTWS_U8 ? 1 : 4;
    const uint64_t *dl, *dn, *de;
    const void* dd;
    double* dout;
    const size_t out_bytes = 10 * sizeof(double) * (size_t)n_edges;
    if ((r = stage_in(h, h->ef_lab, labels, sizeof(uint64_t) * (size_t)N, dev, &dl)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->ef_data, data, es * (size_t)N, dev, &dd)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->ef_nodes, nodes, sizeof(uint64_t) * (size_t)n_nodes, dev, &dn)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->ef_edges, edges, 2 * sizeof(uint64_t) * (size_t)n_edges, dev, &de)) != CTWS_OK) return r;
    if ((r = out_begin(h, h->ef_out, out, out_bytes, dev, &dout)) != CTWS_OK) return r;
    int b = 1;  // bits per rank
    while ((1ll << b) < n_nodes) ++b;
    int eb = 1;  // bits per edge index
    while ((1ll << eb) < n_edges) ++eb;
    if ((r = grow(h, h->ef_red, kRedWords * sizeof(uint64_t))) != CTWS_OK) return r;
    if ((r = grow(h, h->ef_ekeys, sizeof(uint64_t) * (size_t)n_edges)) != CTWS_OK) return r;
    unsigned long long* cnt = (unsigned long long*)h->ef_red.p;
    HIPCHK(hipMemsetAsync(cnt, 0, kRedWords * sizeof(uint64_t), h->stream));
    record(h, 0);
    const unsigned ge = (unsigned)std::min<int64_t>((n_edges + 255) / 256, 8192);
    k_ef_edge_keys<<<ge, 256, 0, h->stream>>>(de, n_edges, dn, n_nodes, b, (uint64_t*)h->ef_ekeys.p,
                                              cnt + kRedBadEdges);
    LAUNCHCHK();
    record(h, 1);
    EfArgs a;
    a.lab = dl;
    a.data = dd;
    a.nz = (uint32_t)nz;
    a.ny = (uint32_t)ny;
    a.nx = (uint32_t)nx;
    a.cz = (uint32_t)cz;
    a.cy = (uint32_t)cy;
    a.cx = (uint32_t)cx;
    a.ignore = ignore_label ? 1 : 0;
    a.tab = dn;
    a.nt = (uint32_t)n_nodes;
    a.b = b;
    a.ekeys = (const uint64_t*)h->ef_ekeys.p;
    a.ne = (uint32_t)n_edges;
    a.count = cnt;
    a.missing = cnt + kRedMissing;
    const int64_t rows = cz * cy;
    // the grid of k_rag_pairs: four workgroups per CU, every wave ends with an append of its own
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, 1024));
    // first capacity: half a key per voxel (a block of fragments emits ~0.38).  The bad-edge
    // count of k_ef_edge_keys is read with the pass's own counters, and not zeroed with them
    EmitCap ecap = {kRedEmit, first_cap(N, 2)};
    Emitted e;
    r = counted_emit(
        h, "edge features", cnt, kRedMissing + 1, kRedBadEdges + 1, &ecap, 1,
        [&] {
            const int r = grow(h, h->ef_keys, sizeof(uint64_t) * (size_t)ecap.cap);
            if (r != CTWS_OK) return r;
            a.keys = (uint64_t*)h->ef_keys.p;
            a.cap = ecap.cap;
            if (data_dtype == CTWS_U8) k_ef_samples<uint8_t><<<g, 256, 0, h->stream>>>(a);
            else k_ef_samples<float><<<g, 256, 0, h->stream>>>(a);
            return CTWS_OK;
        },
        [&](const unsigned long long* w) {
            if (!w[kRedBadEdges]) return CTWS_OK;
            h->err = "edge features: " + std::to_string(w[kRedBadEdges]) +
                     " edges have an endpoint missing from the nodes or are not sorted and unique";
            return CTWS_EINVAL;
        },
        &e);
    if (r != CTWS_OK) return r;
    record(h, 2);
    const int64_t n = (int64_t)e.w[kRedEmit];
    if (n >= (1ll << 31)) {
        h->err = "edge features: 2^31 or more samples in one block";
        return CTWS_EUNSUPPORTED;
    }
    if (n_missing) *n_missing = (int64_t)e.w[kRedMissing];
    const uint64_t* sorted = (const uint64_t*)h->ef_keys.p;
    if (n) {
        size_t tb = 0;
        HIPCHK(sort_keys_u64(nullptr, tb, nullptr, nullptr, n, 32 + eb, h->stream));
        if ((r = grow(h, h->ef_skeys, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
        if ((r = grow(h, h->prim_tmp, tb)) != CTWS_OK) return r;
        HIPCHK(sort_keys_u64(h->prim_tmp.p, tb, (const uint64_t*)h->ef_keys.p, (uint64_t*)h->ef_skeys.p, n,
                             32 + eb, h->stream));
        sorted = (const uint64_t*)h->ef_skeys.p;
    }
    record(h, 3);
    // one wave per edge, four per workgroup
    k_ef_stats<<<(unsigned)((n_edges + 3) / 4), 256, 0, h->stream>>>(sorted, (uint32_t)n, (uint32_t)n_edges, dout);
    LAUNCHCHK();
    record(h, 4);
    if ((r = out_end(h, out, dout, out_bytes, dev)) != CTWS_OK) return r;
    stage_time(h, "ef_edge_keys", 0, 1);
    stage_time(h, "ef_samples", 1, 2);
    stage_time(h, "ef_sort", 2, 3);
    stage_time(h, "ef_stats", 3, 4);
    add_timing(h, "ef_sample_passes", (float)e.passes);
    add_timing(h, "ef_keys", (float)n);
    return CTWS_OK;
}
}  // namespace

extern "C" {

int ctws_edge_features_block(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype, int64_t nz,
                             int64_t ny, int64_t nx, int64_t cz, int64_t cy, int64_t cx, int ignore_label,
                             const uint64_t* nodes, int64_t n_nodes, const uint64_t* edges, int64_t n_edges,
                             double* out, int64_t* n_missing) {
    return edge_features_block(h, labels, data, data_dtype, nz, ny, nx, cz, cy, cx, ignore_label, nodes, n_nodes,
                               edges, n_edges, out, n_missing, false);
}

int ctws_edge_features_block_device(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype,
                                    int64_t nz, int64_t ny, int64_t nx, int64_t cz, int64_t cy, int64_t cx,
                                    int ignore_label, const uint64_t* nodes, int64_t n_nodes, const uint64_t* edges,
                                    int64_t n_edges, double* out, int64_t* n_missing) {
    return edge_features_block(h, labels, data, data_dtype, nz, ny, nx, cz, cy, cx, ignore_label, nodes, n_nodes,
                               edges, n_edges, out, n_missing, true);
}

}  // extern "C"
