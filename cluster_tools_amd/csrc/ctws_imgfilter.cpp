// ctws_imgfilter.cpp — host side of libctws.so: ImageFilter.
#include "ctws_host.h"

using namespace ctws;

// ---- ImageFilter: Gaussian derivative filters of one block (k_imgfilter.hip) -----------------
namespace {
// vigra Kernel1D<double>::initGaussianDerivative(sigma, order) restated (order 0: gaussian_taps):
// the sampled derivative, its mean removed (vigra's DC removal), scaled so that the kernel's order-th
// moment sum_x k(x) (-x)^n / n! is 1 (normalize(1.0, order)); a constant prefactor cancels there
std::vector<double> filter_taps(double sigma, int order) {
    if (order == 0) return gaussian_taps(sigma);
    int radius = (int)((3.0 + 0.5 * order) * sigma + 0.5);
    if (radius == 0) radius = 1;
    const double s2 = sigma * sigma;
    std::vector<double> k;
    double sum = 0.0;
    for (int x = -radius; x <= radius; ++x) {
        const double xx = (double)x * (double)x;
        const double e = std::exp(-xx / (2.0 * s2));
        k.push_back(order == 1 ? -(double)x * e : (xx / s2 - 1.0) * e);
        sum += k.back();
    }
    const double mean = sum / (double)k.size();
    double moment = 0.0;
    for (int x = -radius, i = 0; x <= radius; ++x, ++i) {
        k[(size_t)i] -= mean;
        moment += order == 1 ? k[(size_t)i] * -(double)x : k[(size_t)i] * ((double)x * (double)x) / 2.0;
    }
    for (double& v : k) v = v / moment;
    return k;
}
bool if_sigma_ok(double s) { return s > 0.0 && s * 4.0 + 0.5 < 1073741824.0; }  // (also false for NaN)

using IfKernel = void (*)(IfArgs);
template <int NOUT>
IfKernel if_first_pass(int dtype) {
    return dtype == CTWS_U8    ? &k_if_col<uint8_t, 1, NOUT>
           : dtype == CTWS_U16 ? &k_if_col<uint16_t, 1, NOUT>
           : dtype == CTWS_F32 ? &k_if_col<float, 1, NOUT>
                               : &k_if_col<double, 1, NOUT>;
}

int image_filter(ctws_handle* h, const void* data, int dtype, int64_t nz, int64_t ny, int64_t nx, int filter_id,
                 const double* sigma, int apply_in_2d, int normalize, float* out, bool dev) {
    int r;
    if (!h) return CTWS_EINVAL;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    if (!data || !out || !sigma || nz <= 0 || ny <= 0 || nx <= 0) {
        h->err = "image filter: bad arguments (a non-empty 3-D block, three sigmas and an output)";
        return CTWS_EINVAL;
    }
    if (dtype != CTWS_U8 && dtype != CTWS_U16 && dtype != CTWS_F32 && dtype != CTWS_F64) {
        h->err = "image filter: the block is uint8, uint16, float32 or float64";
        return CTWS_EINVAL;
    }
    if (filter_id != kIfSmooth && filter_id != kIfGradMag && filter_id != kIfLaplace) {
        h->err = "image filter: filter_id is 0 (gaussianSmoothing), 1 (gaussianGradientMagnitude) or 2 "
                 "(laplacianOfGaussian)";
        return CTWS_EINVAL;
    }
    const int a0 = apply_in_2d ? 1 : 0;  // the first filtered axis
    for (int a = a0; a < 3; ++a)
        if (!if_sigma_ok(sigma[a])) {
            h->err = "image filter: every sigma is positive (and below 2^28)";
            return CTWS_EINVAL;
        }
    r = check_extent(h, nz, ny, nx, "image filter", "block", "the kernels index a block with 32 bits");
    if (r != CTWS_OK) return r;
    // the taps: per axis the smoothing taps and, for the derivative filters, those of the order
    constexpr int kSlot = 2 * kIfMaxR + 1;
    const int order = filter_id;  // 0, 1, 2
    std::vector<double> htaps((size_t)6 * kSlot, 0.0);
    int rad[3][2] = {{0, 0}, {0, 0}, {0, 0}}, rmax[3] = {0, 0, 0};
    const int64_t ext[3] = {nz, ny, nx};
    for (int a = a0; a < 3; ++a)
        for (int w = 0; w < (order ? 2 : 1); ++w) {
            const std::vector<double> k = filter_taps(sigma[a], w ? order : 0);
            const int rr = (int)(k.size() / 2);
            rad[a][w] = rr;
            rmax[a] = std::max(rmax[a], rr);
            if (ext[a] < (int64_t)rr + 1) {  // vigra: "kernel longer than line"
                h->err = std::string("image filter: axis ") + "zyx"[a] + " holds " + std::to_string(ext[a]) +
                         " voxels, fewer than the radius " + std::to_string(rr) + " + 1 of the order-" +
                         std::to_string(w ? order : 0) + " taps (sigma " + std::to_string(sigma[a]) + ")";
                return CTWS_EINVAL;
            }
            if (rr > kIfMaxR) {
                h->err = "image filter: a tap radius of " + std::to_string(rr) + " along axis " + "zyx"[a] +
                         ", above the " + std::to_string(kIfMaxR) + " the tiles hold";
                return CTWS_EUNSUPPORTED;
            }
            std::copy(k.begin(), k.end(), htaps.begin() + (size_t)(2 * a + w) * kSlot);
        }
    auto slot = [&](int a, int w) { return (2 * a + w) * kSlot; };
    const size_t es = dtype == CTWS_U8 ? 1 : dtype == CTWS_U16 ? 2 : dtype == CTWS_F32 ? 4 : 8;
    const int64_t N = nz * ny * nx;
    const void* din;
    float* dout;
    if ((r = stage_in(h, h->if_in, data, es * (size_t)N, dev, &din)) != CTWS_OK) return r;
    if ((r = out_begin(h, h->if_out, out, sizeof(float) * (size_t)N, dev, &dout)) != CTWS_OK) return r;
    const size_t fb = sizeof(float) * (size_t)N;
    if ((r = grow(h, h->if_a, (order ? 2 : 1) * fb)) != CTWS_OK) return r;
    if ((r = grow(h, h->if_b, (order ? 3 : 1) * fb)) != CTWS_OK) return r;
    if ((r = grow(h, h->if_taps, sizeof(double) * htaps.size())) != CTWS_OK) return r;
    if ((r = grow(h, h->if_mm, 2 * sizeof(uint32_t))) != CTWS_OK) return r;
    if (h->if_taps_host != htaps) {
        // (a blocking upload: the previous call has ended, nothing reads the taps now)
        h->if_taps_host.clear();
        HIPCHK(hipMemcpy(h->if_taps.p, htaps.data(), sizeof(double) * htaps.size(), hipMemcpyHostToDevice));
        h->if_taps_host = htaps;
    }
    uint32_t* mm = (uint32_t*)h->if_mm.p;
    float* A = (float*)h->if_a.p;
    float* B = (float*)h->if_b.p;
    record(h, 0);
    if (normalize) {
        HIPCHK(hipMemsetAsync(mm, 0xFF, sizeof(uint32_t), h->stream));
        HIPCHK(hipMemsetAsync(mm + 1, 0, sizeof(uint32_t), h->stream));
        const unsigned g = (unsigned)std::min<int64_t>((N + 255) / 256, 512);
        if (dtype == CTWS_U8) k_if_minmax<uint8_t><<<g, 256, 0, h->stream>>>((const uint8_t*)din, N, mm);
        else if (dtype == CTWS_U16) k_if_minmax<uint16_t><<<g, 256, 0, h->stream>>>((const uint16_t*)din, N, mm);
        else if (dtype == CTWS_F32) k_if_minmax<float><<<g, 256, 0, h->stream>>>((const float*)din, N, mm);
        else k_if_minmax<double><<<g, 256, 0, h->stream>>>((const double*)din, N, mm);
        LAUNCHCHK();
    }
    record(h, 1);
    IfArgs base{};
    base.taps = (const double*)h->if_taps.p;
    base.mm = mm;
    base.nz = (int)nz, base.ny = (int)ny, base.nx = (int)nx;
    auto col = [&](IfKernel k, IfArgs& a, int nin, int axis) {
        a.axis = axis;
        a.rmax = rmax[axis];
        const int64_t L = ext[axis], other = axis == 0 ? ny : nz;
        const int64_t tiles = other * ((L + kIfColTL - 1) / kIfColTL) * ((nx + kIfColW - 1) / kIfColW);
        const size_t lds = sizeof(float) * (size_t)nin * (kIfColTL + 2 * a.rmax) * kIfColW;
        k<<<(unsigned)tiles, 256, lds, h->stream>>>(a);
    };
    // the first pass reads the block in its own type, normalized on the fly
    IfArgs p1 = base;
    p1.in[0] = din;
    p1.normalize = normalize ? 1 : 0;
    const int af = a0;  // its axis
    float* first_out = apply_in_2d ? B : A;
    if (order) {  // D, S of the first axis
        p1.out[0] = first_out, p1.out[1] = first_out + N;
        p1.tap[0] = slot(af, 1), p1.rad[0] = rad[af][1];
        p1.tap[1] = slot(af, 0), p1.rad[1] = rad[af][0];
        col(if_first_pass<2>(dtype), p1, 1, af);
    } else {
        p1.out[0] = first_out;
        p1.tap[0] = slot(af, 0), p1.rad[0] = rad[af][0];
        col(if_first_pass<1>(dtype), p1, 1, af);
    }
    LAUNCHCHK();
    record(h, 2);
    if (!apply_in_2d) {  // the y pass of a 3-D filter
        IfArgs p2 = base;
        if (order) {  // S_y D_z, D_y S_z, S_y S_z
            p2.in[0] = A, p2.in[1] = A + N;
            p2.out[0] = B, p2.out[1] = B + N, p2.out[2] = B + 2 * N;
            p2.tap[0] = slot(1, 0), p2.rad[0] = rad[1][0];
            p2.tap[1] = slot(1, 1), p2.rad[1] = rad[1][1];
            p2.tap[2] = slot(1, 0), p2.rad[2] = rad[1][0];
            col(&k_if_col<float, 2, 3>, p2, 2, 1);
        } else {
            p2.in[0] = A;
            p2.out[0] = B;
            p2.tap[0] = slot(1, 0), p2.rad[0] = rad[1][0];
            col(&k_if_col<float, 1, 1>, p2, 1, 1);
        }
        LAUNCHCHK();
    }
    record(h, 3);
    {  // the x pass and the combination: the components in the order z, y, x
        IfArgs p3 = base;
        const int nin = order ? (apply_in_2d ? 2 : 3) : 1;
        for (int s = 0; s < nin; ++s) {
            p3.in[s] = B + (int64_t)s * N;
            const int w = (order && s == nin - 1) ? 1 : 0;  // the last component is the x derivative
            p3.tap[s] = slot(2, w), p3.rad[s] = rad[2][w];
        }
        p3.out[0] = dout;
        p3.rmax = rmax[2];
        p3.combine = filter_id;
        const int64_t wgs = ((nz * ny + 3) / 4) * ((nx + kIfRowW - 1) / kIfRowW);
        const size_t lds = sizeof(float) * 4 * (size_t)nin * (kIfRowW + 2 * p3.rmax);
        const IfKernel k = nin == 1 ? &k_if_row<1> : nin == 2 ? &k_if_row<2> : &k_if_row<3>;
        k<<<(unsigned)wgs, 256, lds, h->stream>>>(p3);
        LAUNCHCHK();
    }
    record(h, 4);
    if ((r = out_end(h, out, dout, fb, dev)) != CTWS_OK) return r;
    stage_time(h, "if_minmax", 0, 1);
    stage_time(h, "if_first", 1, 2);
    stage_time(h, "if_y", 2, 3);
    stage_time(h, "if_x", 3, 4);
    return CTWS_OK;
}
}  // namespace

extern "C" {

int ctws_filter_taps(double sigma, int order, double* out, int* radius) {
    if (!radius || order < 0 || order > 2 || !if_sigma_ok(sigma)) return CTWS_EINVAL;
    const std::vector<double> k = filter_taps(sigma, order);
    *radius = (int)(k.size() / 2);
    if (out) std::copy(k.begin(), k.end(), out);
    return CTWS_OK;
}

int ctws_image_filter(ctws_handle* h, const void* data, int dtype, int64_t nz, int64_t ny, int64_t nx, int filter_id,
                      const double sigma[3], int apply_in_2d, int normalize, float* out) {
    return image_filter(h, data, dtype, nz, ny, nx, filter_id, sigma, apply_in_2d, normalize, out, false);
}

int ctws_image_filter_device(ctws_handle* h, const void* data, int dtype, int64_t nz, int64_t ny, int64_t nx,
                             int filter_id, const double sigma[3], int apply_in_2d, int normalize, float* out) {
    return image_filter(h, data, dtype, nz, ny, nx, filter_id, sigma, apply_in_2d, normalize, out, true);
}

}  // extern "C"
