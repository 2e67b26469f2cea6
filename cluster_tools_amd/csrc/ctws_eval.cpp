// ctws_eval.cpp — host side of libctws.so: the evaluation's contingency table.
#include "ctws_host.h"

using namespace ctws;

extern "C" {

// ---- evaluation: contingency table in HBM (k_eval.hip) ----------------------------------
static int64_t pow2_at_least(int64_t v) {
    int64_t c = 1024;
    while (c < v) c <<= 1;
    return c;
}

int ctws_eval_begin(ctws_handle* h, int64_t cap_labels, int64_t cap_pairs) {
    if (!h || cap_labels < 0 || cap_pairs < 0) return CTWS_EINVAL;
    h->err.clear();
    HIPCHK(hipSetDevice(h->device));
    const int64_t ca = pow2_at_least(2 * std::max<int64_t>(cap_labels, 1));
    const int64_t cp = pow2_at_least(2 * std::max<int64_t>(cap_pairs, 1));
    if (ca > (1ll << 31) || cp > (1ll << 33)) {  // slots + the 2^64 - 1 slot fit the pair key's 32-bit halves
        h->err = "ctws_eval_begin: capacity too large";
        return CTWS_EINVAL;
    }
    int r;
    if ((r = grow(h, h->ev_ka, 8 * (size_t)(ca + 1))) != CTWS_OK || (r = grow(h, h->ev_ca, 8 * (size_t)(ca + 1))) != CTWS_OK ||
        (r = grow(h, h->ev_kb, 8 * (size_t)(ca + 1))) != CTWS_OK || (r = grow(h, h->ev_cb, 8 * (size_t)(ca + 1))) != CTWS_OK ||
        (r = grow(h, h->ev_kp, 8 * (size_t)cp)) != CTWS_OK || (r = grow(h, h->ev_cp, 8 * (size_t)cp)) != CTWS_OK ||
        (r = grow(h, h->ev_state, 16)) != CTWS_OK || (r = grow(h, h->ev_out, 6 * sizeof(double))) != CTWS_OK)
        return r;
    h->ev_cap_a = h->ev_cap_b = ca;
    h->ev_cap_p = cp;
    HIPCHK(hipMemsetAsync(h->ev_ka.p, 0xFF, 8 * (size_t)(ca + 1), h->stream));
    HIPCHK(hipMemsetAsync(h->ev_kb.p, 0xFF, 8 * (size_t)(ca + 1), h->stream));
    HIPCHK(hipMemsetAsync(h->ev_kp.p, 0xFF, 8 * (size_t)cp, h->stream));
    HIPCHK(hipMemsetAsync(h->ev_ca.p, 0, 8 * (size_t)(ca + 1), h->stream));
    HIPCHK(hipMemsetAsync(h->ev_cb.p, 0, 8 * (size_t)(ca + 1), h->stream));
    HIPCHK(hipMemsetAsync(h->ev_cp.p, 0, 8 * (size_t)cp, h->stream));
    HIPCHK(hipMemsetAsync(h->ev_state.p, 0, 16, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTWS_OK;
}

int ctws_eval_add(ctws_handle* h, const uint64_t* seg, const uint64_t* gt, int64_t n, int on_device, int ignore_gt_zero) {
    if (!h || n < 0 || (n > 0 && (!seg || !gt))) return CTWS_EINVAL;
    if (!h->ev_cap_a) {
        h->err = "ctws_eval_add before ctws_eval_begin";
        return CTWS_EINVAL;
    }
    HIPCHK(hipSetDevice(h->device));
    auto launch = [&](const uint64_t* s, const uint64_t* g, int64_t m) -> int {
        const unsigned grid = (unsigned)std::min<int64_t>((m + 255) / 256, 8192);
        k_eval_add<<<grid, 256, 0, h->stream>>>(s, g, m, ignore_gt_zero, (uint64_t*)h->ev_ka.p,
                                                 (unsigned long long*)h->ev_ca.p, h->ev_cap_a, (uint64_t*)h->ev_kb.p,
                                                 (unsigned long long*)h->ev_cb.p, h->ev_cap_b, (uint64_t*)h->ev_kp.p,
                                                 (unsigned long long*)h->ev_cp.p, h->ev_cap_p,
                                                 (unsigned long long*)h->ev_state.p);
        LAUNCHCHK();
        return CTWS_OK;
    };
    int r;
    if (on_device) {
        if ((r = launch(seg, gt, n)) != CTWS_OK) return r;
    } else {
        const int64_t chunk = (int64_t)1 << 25;  // voxels per staged piece (2 x 256 MiB)
        if ((r = grow(h, h->ev_stage, 16 * (size_t)std::min(chunk, std::max<int64_t>(n, 1)))) != CTWS_OK) return r;
        uint64_t* ds = (uint64_t*)h->ev_stage.p;
        for (int64_t o = 0; o < n; o += chunk) {
            const int64_t m = std::min(chunk, n - o);
            uint64_t* dg = ds + std::min(chunk, std::max<int64_t>(n, 1));
            HIPCHK(hipMemcpyAsync(ds, seg + o, 8 * (size_t)m, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipMemcpyAsync(dg, gt + o, 8 * (size_t)m, hipMemcpyHostToDevice, h->stream));
            if ((r = launch(ds, dg, m)) != CTWS_OK) return r;
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTWS_OK;
}

int ctws_eval_end(ctws_handle* h, double* scores, int64_t* n_points) {
    if (!h || !scores) return CTWS_EINVAL;
    if (!h->ev_cap_a) {
        h->err = "ctws_eval_end before ctws_eval_begin";
        return CTWS_EINVAL;
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemsetAsync(h->ev_out.p, 0, 6 * sizeof(double), h->stream));
    const unsigned grid = (unsigned)std::min<int64_t>((std::max(h->ev_cap_a, h->ev_cap_p) + 255) / 256, 4096);
    k_eval_reduce<<<grid, 256, 0, h->stream>>>((const uint64_t*)h->ev_ka.p, (const unsigned long long*)h->ev_ca.p,
                                               h->ev_cap_a, (const uint64_t*)h->ev_kb.p,
                                               (const unsigned long long*)h->ev_cb.p, h->ev_cap_b,
                                               (const uint64_t*)h->ev_kp.p, (const unsigned long long*)h->ev_cp.p,
                                               h->ev_cap_p, (const unsigned long long*)h->ev_state.p,
                                               (double*)h->ev_out.p);
    LAUNCHCHK();
    double v[6];
    unsigned long long st[2];
    HIPCHK(hipMemcpyAsync(v, h->ev_out.p, sizeof(v), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(st, h->ev_state.p, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (st[1]) {
        h->err = "contingency hash table full: call ctws_eval_begin with larger capacities";
        return CTWS_EUNSUPPORTED;
    }
    const double n = (double)st[0];
    if (n_points) *n_points = (int64_t)st[0];
    // validation_utils.py:60-76 (a = gt, b = seg) and :178-198
    scores[0] = v[1] - v[2];  // vi split
    scores[1] = v[0] - v[2];  // vi merge
    const double prec = v[4] > 0 ? v[5] / v[4] : 0.0, rec = v[3] > 0 ? v[5] / v[3] : 0.0;
    const double ari = (prec + rec) > 0 ? 2 * prec * rec / (prec + rec) : 0.0;
    scores[2] = 1.0 - ari;
    scores[3] = n > 0 ? 1.0 - (v[3] + v[4] - 2 * v[5]) / (n * n) : 1.0;
    return CTWS_OK;
}

}  // extern "C"
