// ctws_host.cpp — host side of libctws.so: what ctws_host.h declares for every translation unit.
#include "ctws_host.h"

namespace ctws {

int grow(ctws_handle* h, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes) return CTWS_OK;
    if (b.p) hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
    if (hipMalloc(&b.p, std::max<size_t>(bytes, 16)) != hipSuccess) {
        h->err = "hipMalloc staging failed (" + std::to_string(bytes) + " bytes)";
        return CTWS_ENOMEM;
    }
    b.bytes = bytes;
    return CTWS_OK;
}

void record(ctws_handle* h, size_t idx) {
    while (h->events.size() <= idx) {
        hipEvent_t e;
        hipEventCreate(&e);
        h->events.push_back(e);
    }
    hipEventRecord(h->events[idx], h->stream);
}

void add_timing(ctws_handle* h, const char* name, float v) {
    for (auto& t : h->timings)
        if (std::strcmp(t.first, name) == 0) {
            t.second += v;
            return;
        }
    h->timings.push_back({name, v});
}

void set_timing(ctws_handle* h, const char* name, float v) {
    for (auto& t : h->timings)
        if (std::strcmp(t.first, name) == 0) {
            t.second = v;
            return;
        }
    h->timings.push_back({name, v});
}

void stage_time(ctws_handle* h, const char* name, size_t a, size_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->events[a], h->events[b]) == hipSuccess) add_timing(h, name, ms);
}

hipError_t copy_pieces(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    constexpr size_t kPiece = (size_t)1 << 30;
    for (size_t o = 0; o < bytes; o += kPiece) {
        const hipError_t e = hipMemcpyAsync((char*)dst + o, (const char*)src + o, std::min(kPiece, bytes - o), kind, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

std::vector<double> gaussian_taps(double sigma) {
    std::vector<double> k;
    if (sigma > 0.0) {
        const double sigma2 = -0.5 / sigma / sigma;
        const double norm = 1.0 / (std::sqrt(2.0 * M_PI) * sigma);
        int radius = (int)(3.0 * sigma + 0.5);
        if (radius == 0) radius = 1;
        for (double x = -(double)radius; x <= (double)radius; ++x) {
            const double x2 = x * x;
            k.push_back(norm * std::exp(x2 * sigma2));
        }
    } else {
        k.push_back(1.0);
    }
    double sum = 0.0;
    for (double v : k) sum += v;
    sum = 1.0 / sum;
    for (double& v : k) v = v * sum;
    return k;
}

int call_begin(ctws_handle* h) {
    h->err.clear();
    h->timings.clear();
    HIPCHK(hipSetDevice(h->device));
    return CTWS_OK;
}

int check_extent(ctws_handle* h, int64_t nz, int64_t ny, int64_t nx, const char* what, const char* unit,
                 const char* why) {
    constexpr int64_t kMax = 1ll << 31;
    if (nz >= kMax || ny >= kMax || nx >= kMax || nz * ny >= kMax || nz * ny * nx >= kMax) {
        h->err = std::string(what) + ": 2^31 or more voxels in one " + unit + " (" + why + ")";
        return CTWS_EUNSUPPORTED;
    }
    return CTWS_OK;
}

int out_end(ctws_handle* h, void* dst, const void* d, size_t bytes, bool dev) {
    if (!dev) HIPCHK(copy_pieces(dst, d, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTWS_OK;
}

unsigned long long first_cap(int64_t n, int64_t div) { return (unsigned long long)std::max<int64_t>(64, n / div); }

int runs_within(ctws_handle* h, const char* what, unsigned long long runs, int64_t lo, int64_t n) {
    if (runs >= (unsigned long long)lo && runs <= (unsigned long long)n) return CTWS_OK;
    h->err = std::string(what) + ": the kernel counted " + std::to_string(runs) + " runs in " + std::to_string(n) +
             " voxels";
    return CTWS_EHIP;
}

int sort_by_id(ctws_handle* h, const char* what, const uint64_t* ids, const uint64_t* recs, int64_t n,
               unsigned long long vmax, size_t ev, ById* o) {
    if (vmax >= (1ull << 53)) {
        h->err = std::string(what) + ": an id of 2^53 or more (" + std::to_string(vmax) +
                 ") has no exact place in the float64 rows";
        return CTWS_EUNSUPPORTED;
    }
    int bits = 1;
    while (bits < 53 && (1ull << bits) <= vmax) ++bits;
    int r;
    const size_t nb = sizeof(uint64_t) * (size_t)n;
    size_t tb_sort = 0, tb_rle = 0;
    HIPCHK(sort_pairs_u64(nullptr, tb_sort, nullptr, nullptr, nullptr, nullptr, n, bits, h->stream));
    HIPCHK(runs_u64(nullptr, tb_rle, nullptr, nullptr, nullptr, nullptr, n, h->stream));
    if ((r = grow(h, h->rg_skeys, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_sw, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_keys, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_sum, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->prim_tmp, std::max(tb_sort, tb_rle))) != CTWS_OK) return r;
    o->sids = (uint64_t*)h->rg_skeys.p;
    o->srecs = (uint64_t*)h->rg_sw.p;
    o->uniq = (uint64_t*)h->rg_keys.p;
    o->counts = (uint64_t*)h->rg_sum.p;
    uint64_t* nruns = (uint64_t*)h->rg_red.p + kRedRuns;
    HIPCHK(sort_pairs_u64(h->prim_tmp.p, tb_sort, ids, o->sids, recs, o->srecs, n, bits, h->stream));
    HIPCHK(runs_u64(h->prim_tmp.p, tb_rle, o->sids, o->uniq, o->counts, nruns, n, h->stream));
    record(h, ev);
    unsigned long long runs = 0;
    HIPCHK(hipMemcpyAsync(&runs, nruns, sizeof(runs), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (runs == 0 || runs > (unsigned long long)n) {
        h->err = std::string(what) + ": " + std::to_string(runs) + " ids from " + std::to_string(n) + " runs";
        return CTWS_EHIP;
    }
    o->m = (int64_t)runs;
    return CTWS_OK;
}

}  // namespace ctws
