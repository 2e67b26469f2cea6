// ctws_threshcc.cpp — host side of libctws.so: ThresholdedComponentsWorkflow.
#include "ctws_host.h"

using namespace ctws;

// ---- ThresholdedComponentsWorkflow: BlockComponents (k_threshcc.hip) -----------------------
namespace {
size_t tc_dtype_size(int dt) {
    switch (dt) {
        case CTWS_U8: case CTWS_I8: return 1;
        case CTWS_U16: case CTWS_I16: return 2;
        case CTWS_F32: case CTWS_I32: case CTWS_U32: return 4;
        case CTWS_F64: case CTWS_I64: case CTWS_U64: return 8;
        default: return 0;
    }
}
// dispatch a k_tc_* template over the dataset dtype (float32 is the caller's own case)
template <class F>
void tc_dispatch(int dt, F f) {
    switch (dt) {
        case CTWS_U8: f((const uint8_t*)nullptr); break;
        case CTWS_I8: f((const int8_t*)nullptr); break;
        case CTWS_U16: f((const uint16_t*)nullptr); break;
        case CTWS_I16: f((const int16_t*)nullptr); break;
        case CTWS_U32: f((const uint32_t*)nullptr); break;
        case CTWS_I32: f((const int32_t*)nullptr); break;
        case CTWS_U64: f((const uint64_t*)nullptr); break;
        case CTWS_I64: f((const int64_t*)nullptr); break;
        case CTWS_F64: f((const double*)nullptr); break;
        default: break;
    }
}
}  // namespace

extern "C" {

int ctws_threshold_components(ctws_handle* h, const float* input, const uint8_t* mask, int64_t nz, int64_t ny,
                              int64_t nx, int on_device, int mode, double threshold, int normalize, uint64_t* out,
                              int64_t* n_labels) {
    return ctws_threshold_components_ex(h, input, CTWS_F32, mask, nz, ny, nx, on_device, mode, threshold, normalize,
                                        0.0, out, n_labels);
}

int ctws_threshold_components_ex(ctws_handle* h, const void* input, int dtype, const uint8_t* mask, int64_t nz,
                                 int64_t ny, int64_t nx, int on_device, int mode, double threshold, int normalize,
                                 double sigma, uint64_t* out, int64_t* n_labels) {
    if (!h || !n_labels || nz < 0 || ny < 0 || nx < 0 || mode < 0 || mode > 2 || !(sigma >= 0.0)) return CTWS_EINVAL;
    const size_t esz = tc_dtype_size(dtype);
    if (!esz) {
        h->err = "ctws_threshold_components_ex: unsupported dtype";
        return CTWS_EINVAL;
    }
    const int64_t n = nz * ny * nx;
    if ((!input || !out) && n > 0) return CTWS_EINVAL;
    h->err.clear();
    HIPCHK(hipSetDevice(h->device));
    *n_labels = 0;
    if (n == 0) return CTWS_OK;
    if (n >= (int64_t)kNoParent || nz > INT32_MAX || ny > INT32_MAX || nx > INT32_MAX) {
        h->err = "ctws_threshold_components: block too large (needs < 2^32 - 1 voxels)";
        return CTWS_EINVAL;
    }
    std::vector<double> taps;
    if (sigma > 0.0) {
        taps = gaussian_taps(sigma);
        const int64_t rad = (int64_t)taps.size() / 2;
        if (nz < rad + 1 || ny < rad + 1 || nx < rad + 1) {  // vigra: "kernel longer than line"
            h->err = "ctws_threshold_components_ex: block shorter than the Gaussian radius + 1 along an axis";
            return CTWS_EINVAL;
        }
    }
    int r;
    const void* dsrc = input;
    const uint8_t* dmask = mask;
    uint64_t* dout = out;
    if (!on_device) {
        if ((r = grow(h, h->tc_raw, esz * (size_t)n)) != CTWS_OK) return r;
        if ((r = grow(h, h->tc_out, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
        HIPCHK(hipMemcpyAsync(h->tc_raw.p, input, esz * (size_t)n, hipMemcpyHostToDevice, h->stream));
        dsrc = h->tc_raw.p;
        dout = (uint64_t*)h->tc_out.p;
        if (mask) {
            if ((r = grow(h, h->tc_mask, (size_t)n)) != CTWS_OK) return r;
            HIPCHK(hipMemcpyAsync(h->tc_mask.p, mask, (size_t)n, hipMemcpyHostToDevice, h->stream));
            dmask = (const uint8_t*)h->tc_mask.p;
        }
    }
    const int64_t nw = (n + 63) / 64, nc = (nw + 255) / 256;
    if ((r = grow(h, h->tc_P, sizeof(uint32_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->tc_bits, sizeof(uint64_t) * (size_t)nw)) != CTWS_OK) return r;
    if ((r = grow(h, h->tc_cnt, sizeof(uint32_t) * (size_t)nc)) != CTWS_OK) return r;
    if ((r = grow(h, h->tc_offs, sizeof(uint64_t) * (size_t)(nc + 1))) != CTWS_OK) return r;
    if ((r = grow(h, h->tc_woff, sizeof(uint32_t) * (size_t)nw)) != CTWS_OK) return r;
    if ((r = grow(h, h->tc_red, 4 * sizeof(uint32_t))) != CTWS_OK) return r;
    uint32_t* red = (uint32_t*)h->tc_red.p;  // [0] min, [1] max (ordered float bits), [2] any member
    const uint32_t init[3] = {0xFFFFFFFFu, 0u, 0u};
    HIPCHK(hipMemcpyAsync(red, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
    const unsigned gs = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);  // grid of the streaming passes
    const unsigned gm = (unsigned)std::min<int64_t>((n + 4095) / 4096, 256);  // k_tc_minmax
    TcParams p;
    p.nz = (int)nz;
    p.ny = (int)ny;
    p.nx = (int)nx;
    p.mode = mode;
    p.normalize = normalize ? 1 : 0;
    p.thr = (float)threshold;
    const float* din = (const float*)dsrc;  // the float32 values k_tc_tile thresholds
    const bool raw_cmp = !normalize && sigma == 0.0 && dtype != CTWS_F32;
    if (raw_cmp || dtype != CTWS_F32) {
        if ((r = grow(h, h->tc_in, sizeof(float) * (size_t)n)) != CTWS_OK) return r;
        float* f = (float*)h->tc_in.p;
        if (raw_cmp) {
            // numpy's float64 comparison of the raw values; k_tc_tile tests the 0 / 1 result
            tc_dispatch(dtype, [&](auto tp) {
                using T = std::remove_cv_t<std::remove_pointer_t<decltype(tp)>>;
                k_tc_raw_members<T><<<gs, 256, 0, h->stream>>>((const T*)dsrc, n, mode, threshold, f);
            });
            p.mode = 0;
            p.thr = 0.5f;
        } else {
            tc_dispatch(dtype, [&](auto tp) {
                using T = std::remove_cv_t<std::remove_pointer_t<decltype(tp)>>;
                k_tc_to_f32<T><<<gs, 256, 0, h->stream>>>((const T*)dsrc, n, f);
            });
        }
        LAUNCHCHK();
        din = f;
    }
    if (sigma > 0.0) {
        // x (float32) -> [normalize] -> Gaussian z, y, x -> normalized by k_tc_tile
        if ((r = grow(h, h->tc_tmp, sizeof(float) * (size_t)n)) != CTWS_OK) return r;
        if ((r = grow(h, h->tc_taps, sizeof(double) * taps.size())) != CTWS_OK) return r;
        if (din == (const float*)dsrc) {  // float32 input: work on a copy, the caller's buffer is const
            if ((r = grow(h, h->tc_in, sizeof(float) * (size_t)n)) != CTWS_OK) return r;
            HIPCHK(hipMemcpyAsync(h->tc_in.p, din, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, h->stream));
            din = (const float*)h->tc_in.p;
        }
        float* a = (float*)h->tc_in.p;
        float* b = (float*)h->tc_tmp.p;
        if (normalize) {
            k_tc_minmax<<<gm, 256, 0, h->stream>>>(a, n, red);
            k_tc_normalize<<<gs, 256, 0, h->stream>>>(a, n, red);
            HIPCHK(hipMemcpyAsync(red, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
        }
        // (pageable upload: the host vector is gone after this call returns, the copy is not)
        HIPCHK(hipMemcpy(h->tc_taps.p, taps.data(), sizeof(double) * taps.size(), hipMemcpyHostToDevice));
        const int rad = (int)taps.size() / 2;
        for (int axis = 0; axis < 3; ++axis) {
            k_tc_gauss<<<gs, 256, 0, h->stream>>>(a, b, (int)nz, (int)ny, (int)nx, axis,
                                                  (const double*)h->tc_taps.p, rad);
            std::swap(a, b);
        }
        LAUNCHCHK();
        din = a;
        p.normalize = 1;  // vu.normalize of the smoothed block
    }
    if (p.normalize) {
        if (reinterpret_cast<uintptr_t>(din) % 16 != 0) {
            h->err = "ctws_threshold_components: input not 16-byte aligned";
            return CTWS_EINVAL;
        }
        k_tc_minmax<<<gm, 256, 0, h->stream>>>(din, n, red);
    }
    const int64_t tiles = ((nx + 63) / 64) * ((ny + 7) / 8) * ((nz + 7) / 8);
    uint32_t* P = (uint32_t*)h->tc_P.p;
    k_tc_tile<<<(unsigned)tiles, 256, 0, h->stream>>>(din, dmask, p, red, P, red + 2);
    LAUNCHCHK();
    uint32_t any = 0;
    HIPCHK(hipMemcpyAsync(&any, red + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!any) return CTWS_OK;  // an empty block: no labels, the output is not written
    k_tc_merge<<<(unsigned)std::min<int64_t>(tiles, 4096), 256, 0, h->stream>>>(p, P);
    const unsigned gv = (unsigned)((n + 255) / 256);
    k_tc_roots<<<gv, 256, 0, h->stream>>>(P, n, (uint64_t*)h->tc_bits.p);
    k_bits_chunk_count<<<(unsigned)nc, 256, 0, h->stream>>>((const uint64_t*)h->tc_bits.p, nw,
                                                           (uint32_t*)h->tc_cnt.p);
    k_scan_chunks<<<1, 256, 0, h->stream>>>((const uint32_t*)h->tc_cnt.p, nc, (uint64_t*)h->tc_offs.p);
    k_tc_wordoff<<<(unsigned)nc, 256, 0, h->stream>>>((const uint64_t*)h->tc_bits.p, nw,
                                                     (const uint64_t*)h->tc_offs.p, (uint32_t*)h->tc_woff.p);
    k_tc_label<<<gv, 256, 0, h->stream>>>(P, n, (const uint64_t*)h->tc_bits.p, (const uint32_t*)h->tc_woff.p, dout);
    LAUNCHCHK();
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, (uint64_t*)h->tc_offs.p + nc, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    if (!on_device) HIPCHK(hipMemcpyAsync(out, dout, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *n_labels = (int64_t)total;
    return CTWS_OK;
}


// ---- ThresholdedComponentsWorkflow: MergeAssignments (host) --------------------------------
// nifty.ufd.boost_ufd(n).merge(pairs); find(arange(n)) (merge_assignments.py:125-130): boost's
// disjoint_sets with union by rank -- link(find(a), find(b)) puts the root of lower rank under
// the other and, at equal ranks, the first root under the second (whose rank grows).  The
// representatives depend on the merge order, so this stays a sequential pass over the pairs.
int ctws_ufd_find(int64_t n, const uint64_t* pairs, int64_t n_pairs, uint64_t* out) {
    if (n < 0 || n_pairs < 0 || (!out && n > 0) || (!pairs && n_pairs > 0)) return CTWS_EINVAL;
    std::vector<uint64_t> parent((size_t)n);
    std::vector<uint8_t> rank((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) parent[(size_t)i] = (uint64_t)i;
    auto find = [&](uint64_t a) {
        uint64_t r = a;
        while (parent[r] != r) r = parent[r];
        while (parent[a] != r) {  // full path compression (boost's default find)
            const uint64_t nx = parent[a];
            parent[a] = r;
            a = nx;
        }
        return r;
    };
    for (int64_t k = 0; k < n_pairs; ++k) {
        const uint64_t a = pairs[2 * k], b = pairs[2 * k + 1];
        if (a >= (uint64_t)n || b >= (uint64_t)n) return CTWS_EINVAL;
        const uint64_t i = find(a), j = find(b);
        if (i == j) continue;
        if (rank[i] > rank[j]) {
            parent[j] = i;
        } else {
            parent[i] = j;
            if (rank[i] == rank[j]) ++rank[j];
        }
    }
    for (int64_t i = 0; i < n; ++i) out[i] = find((uint64_t)i);
    return CTWS_OK;
}

}  // extern "C"
