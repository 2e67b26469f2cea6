// ctws_relabel.cpp — host side of libctws.so: RelabelWorkflow (sorted uniques, assignment-table lookup).
#include "ctws_host.h"

using namespace ctws;

namespace ctws {
int unique_sorted(ctws_handle* h, const uint64_t* dl, int64_t n, int on_device, uint64_t* out, uint64_t* counts,
                  int64_t cap, int64_t* n_unique) {
    if (n >= (1ll << 31)) {
        h->err = "unique: more than 2^31 - 1 labels in one call";
        return CTWS_EUNSUPPORTED;
    }
    int r;
    size_t tb_sort = 0, tb_rle = 0;
    HIPCHK(sort_keys_u64(nullptr, tb_sort, dl, nullptr, n, 64, h->stream));
    HIPCHK(runs_u64(nullptr, tb_rle, nullptr, nullptr, nullptr, nullptr, n, h->stream));
    if ((r = grow(h, h->rl_sorted, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->rl_uniq, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->rl_counts, sizeof(uint64_t) * (size_t)n + 64)) != CTWS_OK) return r;
    if ((r = grow(h, h->prim_tmp, std::max(tb_sort, tb_rle))) != CTWS_OK) return r;
    uint64_t* sorted = (uint64_t*)h->rl_sorted.p;
    uint64_t* uniq = (uint64_t*)h->rl_uniq.p;
    uint64_t* cnt = (uint64_t*)h->rl_counts.p;
    uint64_t* nruns = cnt + n;  // (the counts buffer has 64 spare bytes)
    HIPCHK(sort_keys_u64(h->prim_tmp.p, tb_sort, dl, sorted, n, 64, h->stream));
    HIPCHK(runs_u64(h->prim_tmp.p, tb_rle, sorted, uniq, cnt, nruns, n, h->stream));
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, nruns, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *n_unique = (int64_t)total;
    if ((int64_t)total > cap) {
        h->err = "unique: output capacity too small";
        return CTWS_EINVAL;
    }
    const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (total) {
        HIPCHK(hipMemcpyAsync(out, uniq, sizeof(uint64_t) * total, k, h->stream));
        if (counts) HIPCHK(hipMemcpyAsync(counts, cnt, sizeof(uint64_t) * total, k, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTWS_OK;
}
}  // namespace ctws

namespace {
const uint64_t* stage_labels(ctws_handle* h, const uint64_t* labels, int64_t n, int on_device, int* r) {
    *r = CTWS_OK;
    if (on_device) return labels;
    if ((*r = grow(h, h->rl_lab, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return nullptr;
    if (hipMemcpyAsync(h->rl_lab.p, labels, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream) !=
        hipSuccess) {
        h->err = "unique: label upload failed";
        *r = CTWS_EHIP;
        return nullptr;
    }
    return (const uint64_t*)h->rl_lab.p;
}
}  // namespace

extern "C" {

// ---- RelabelWorkflow kernels (k_relabel.hip) ----------------------------------------------
int ctws_unique_counts_u64(ctws_handle* h, const uint64_t* labels, int64_t n, int on_device, uint64_t* out,
                           uint64_t* counts, int64_t cap, int64_t* n_unique) {
    if (!h || (!labels && n > 0) || n < 0 || !n_unique || cap < 0 || ((!out || !counts) && cap > 0))
        return CTWS_EINVAL;
    h->err.clear();
    HIPCHK(hipSetDevice(h->device));
    *n_unique = 0;
    if (n == 0) return CTWS_OK;
    int r;
    const uint64_t* dl = stage_labels(h, labels, n, on_device, &r);
    if (r != CTWS_OK) return r;
    return unique_sorted(h, dl, n, on_device, out, counts, cap, n_unique);
}

int ctws_unique_u64(ctws_handle* h, const uint64_t* labels, int64_t n, int on_device, uint64_t* out, int64_t cap,
                    int64_t* n_unique) {
    if (!h || (!labels && n > 0) || n < 0 || !n_unique || cap < 0 || (!out && cap > 0)) return CTWS_EINVAL;
    h->err.clear();
    HIPCHK(hipSetDevice(h->device));
    *n_unique = 0;
    if (n == 0) return CTWS_OK;
    int r;
    const uint64_t* dl = stage_labels(h, labels, n, on_device, &r);
    if (r != CTWS_OK) return r;
    if ((r = grow(h, h->rl_red, 4 * sizeof(uint64_t))) != CTWS_OK) return r;
    unsigned long long* red = (unsigned long long*)h->rl_red.p;
    const unsigned long long init[3] = {~0ull, 0ull, 0ull};
    HIPCHK(hipMemcpyAsync(red, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
    const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    k_u64_range<<<g, 256, 0, h->stream>>>(dl, n, red);
    LAUNCHCHK();
    unsigned long long hr[3];
    HIPCHK(hipMemcpyAsync(hr, red, sizeof(hr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const bool has_nz = hr[1] != 0ull;  // (the min stays ~0 when every nonzero label is 2^64 - 1)
    const int64_t first = hr[2] ? 1 : 0;
    int64_t total = first;
    if (has_nz) {
        const uint64_t lo = hr[0], span = hr[1] - hr[0];  // (+ 1 below; 0 .. 2^64 - 1 would wrap)
        // the bitmap (span / 8 bytes) only while it is no larger than sorting the labels would
        // need (~16 bytes each) or small anyway; otherwise sort (any value range)
        if (span >= (1ull << 35) || span / 64 + 1 > (uint64_t)std::max<int64_t>(2 * n, 1 << 20))
            return unique_sorted(h, dl, n, on_device, out, nullptr, cap, n_unique);
        const int64_t nw = (int64_t)(span / 64 + 1), nc = (nw + 255) / 256;
        if ((r = grow(h, h->rl_bits, sizeof(uint64_t) * (size_t)nw)) != CTWS_OK) return r;
        if ((r = grow(h, h->rl_cnt, sizeof(uint32_t) * (size_t)nc)) != CTWS_OK) return r;
        if ((r = grow(h, h->rl_offs, sizeof(uint64_t) * (size_t)(nc + 1))) != CTWS_OK) return r;
        HIPCHK(hipMemsetAsync(h->rl_bits.p, 0, sizeof(uint64_t) * (size_t)nw, h->stream));
        k_u64_bits<<<g, 256, 0, h->stream>>>(dl, n, lo, (unsigned long long*)h->rl_bits.p);
        k_bits_chunk_count<<<(unsigned)nc, 256, 0, h->stream>>>((const uint64_t*)h->rl_bits.p, nw,
                                                               (uint32_t*)h->rl_cnt.p);
        k_scan_chunks<<<1, 256, 0, h->stream>>>((const uint32_t*)h->rl_cnt.p, nc, (uint64_t*)h->rl_offs.p);
        LAUNCHCHK();
        uint64_t cnt = 0;
        HIPCHK(hipMemcpyAsync(&cnt, (uint64_t*)h->rl_offs.p + nc, sizeof(uint64_t), hipMemcpyDeviceToHost,
                              h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        total += (int64_t)cnt;
        *n_unique = total;
        if (total > cap) {
            h->err = "ctws_unique_u64: output capacity too small";
            return CTWS_EINVAL;
        }
        uint64_t* dout = out;
        if (!on_device) {
            if ((r = grow(h, h->rl_out, sizeof(uint64_t) * (size_t)total)) != CTWS_OK) return r;
            dout = (uint64_t*)h->rl_out.p;
        }
        k_bits_compact<<<(unsigned)nc, 256, 0, h->stream>>>((const uint64_t*)h->rl_bits.p, nw,
                                                           (const uint64_t*)h->rl_offs.p, lo, (uint64_t)first, dout);
        LAUNCHCHK();
        if (first) HIPCHK(hipMemsetAsync(dout, 0, sizeof(uint64_t), h->stream));
        if (!on_device)
            HIPCHK(hipMemcpyAsync(out, dout, sizeof(uint64_t) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return CTWS_OK;
    }
    *n_unique = total;  // only zeros
    if (total > cap) {
        h->err = "ctws_unique_u64: output capacity too small";
        return CTWS_EINVAL;
    }
    if (on_device) HIPCHK(hipMemsetAsync(out, 0, sizeof(uint64_t), h->stream));
    else out[0] = 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTWS_OK;
}

int ctws_set_table_u64(ctws_handle* h, const uint64_t* keys, const uint64_t* values, int64_t n_table) {
    if (!h || n_table < 0 || ((!keys || !values) && n_table > 0)) return CTWS_EINVAL;
    h->err.clear();
    HIPCHK(hipSetDevice(h->device));
    int r;
    if ((r = grow(h, h->rl_keys, sizeof(uint64_t) * (size_t)std::max<int64_t>(1, n_table))) != CTWS_OK) return r;
    if ((r = grow(h, h->rl_vals, sizeof(uint64_t) * (size_t)std::max<int64_t>(1, n_table))) != CTWS_OK) return r;
    if (n_table) {
        HIPCHK(hipMemcpyAsync(h->rl_keys.p, keys, sizeof(uint64_t) * (size_t)n_table, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->rl_vals.p, values, sizeof(uint64_t) * (size_t)n_table, hipMemcpyHostToDevice,
                              h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->rl_ntable = n_table;
    return CTWS_OK;
}

int ctws_lookup_u64(ctws_handle* h, uint64_t* labels, int64_t n, int on_device, const uint64_t* keys,
                    const uint64_t* values, int64_t n_table, int64_t* n_missing) {
    if (!h || (!labels && n > 0) || n < 0) return CTWS_EINVAL;
    const bool resident = !keys && !values;
    if (!resident && (n_table < 0 || ((!keys || !values) && n_table > 0))) return CTWS_EINVAL;
    h->err.clear();
    HIPCHK(hipSetDevice(h->device));
    if (n_missing) *n_missing = 0;
    if (n == 0) return CTWS_OK;
    int r;
    if (resident) {
        n_table = h->rl_ntable;
    } else if (!on_device) {
        // host table: upload it as the resident one
        if ((r = ctws_set_table_u64(h, keys, values, n_table)) != CTWS_OK) return r;
    }
    const uint64_t* dk = (resident || !on_device) ? (const uint64_t*)h->rl_keys.p : keys;
    const uint64_t* dv = (resident || !on_device) ? (const uint64_t*)h->rl_vals.p : values;
    uint64_t* dl = labels;
    if (!on_device) {
        if ((r = grow(h, h->rl_lab, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
        dl = (uint64_t*)h->rl_lab.p;
        HIPCHK(hipMemcpyAsync(dl, labels, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    }
    if ((r = grow(h, h->rl_red, 4 * sizeof(uint64_t))) != CTWS_OK) return r;
    unsigned long long* miss = (unsigned long long*)h->rl_red.p + 3;
    HIPCHK(hipMemsetAsync(miss, 0, sizeof(uint64_t), h->stream));
    const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    k_u64_lookup<<<g, 256, 0, h->stream>>>(dl, n, dk, dv, n_table, miss);
    LAUNCHCHK();
    unsigned long long hm = 0;
    HIPCHK(hipMemcpyAsync(&hm, miss, sizeof(hm), hipMemcpyDeviceToHost, h->stream));
    if (!on_device) HIPCHK(hipMemcpyAsync(labels, dl, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (n_missing) *n_missing = (int64_t)hm;
    return CTWS_OK;
}

}  // extern "C"
