// ctws_downscale.cpp — host side of libctws.so: DownscalingWorkflow.
#include "ctws_host.h"

using namespace ctws;

// ---- DownscalingWorkflow: block reduction of one block (k_downscale.hip) ---------------------
namespace {
using DsKernel = void (*)(DownscaleArgs);
template <class T>
DsKernel ds_kernel(int func, int variant) {  // variant 0: any factor, 1: (1, 2, 2), 2: (2, 2, 2)
    static const DsKernel table[3][3] = {
        {&k_downscale_cell<T, kDsMean>, &k_downscale_vec<T, kDsMean, 1>, &k_downscale_vec<T, kDsMean, 2>},
        {&k_downscale_cell<T, kDsMax>, &k_downscale_vec<T, kDsMax, 1>, &k_downscale_vec<T, kDsMax, 2>},
        {&k_downscale_cell<T, kDsMin>, &k_downscale_vec<T, kDsMin, 1>, &k_downscale_vec<T, kDsMin, 2>}};
    return table[func][variant];
}

int downscale_block(ctws_handle* h, const void* input, int dtype, int64_t nz, int64_t ny, int64_t nx,
                    const int64_t factors[3], int func, void* out, int64_t oz, int64_t oy, int64_t ox,
                    int* any_nonzero, bool dev) {
    int r;
    if (!h) return CTWS_EINVAL;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    if (!input || !out || !factors || !any_nonzero || nz <= 0 || ny <= 0 || nx <= 0) {
        h->err = "downscale: bad arguments (a non-empty 3-D block, factors, an output and a flag)";
        return CTWS_EINVAL;
    }
    *any_nonzero = 0;
    if (dtype != CTWS_U8 && dtype != CTWS_U16 && dtype != CTWS_F32 && dtype != CTWS_F64) {
        h->err = "downscale: the block is uint8, uint16, float32 or float64";
        return CTWS_EINVAL;
    }
    if (func != kDsMean && func != kDsMax && func != kDsMin) {
        h->err = "downscale: func is 0 (mean), 1 (max) or 2 (min)";
        return CTWS_EINVAL;
    }
    for (int d = 0; d < 3; ++d)
        if (factors[d] < 1 || factors[d] > 8) {
            h->err = "downscale: every factor lies in 1..8";
            return CTWS_EINVAL;
        }
    r = check_extent(h, nz, ny, nx, "downscale", "block", "the kernels index a block with 32 bits");
    if (r != CTWS_OK) return r;
    const int64_t fz = factors[0], fy = factors[1], fx = factors[2], n = fz * fy * fx;
    if (oz != (nz + fz - 1) / fz || oy != (ny + fy - 1) / fy || ox != (nx + fx - 1) / fx) {
        h->err = "downscale: the output extents are ceil(n / f) per axis";
        return CTWS_EINVAL;
    }
    if (func == kDsMean && dtype == CTWS_U16 && n * 65535 >= (1ll << 24)) {
        h->err = "downscale: the mean of " + std::to_string(n) + " uint16 voxels: the cell's sum can reach 2^24, where "
                 "float32 no longer holds it exactly and the reference's summation order would decide the result";
        return CTWS_EUNSUPPORTED;
    }
    const size_t es = dtype == CTWS_U8 ? 1 : dtype == CTWS_U16 ? 2 : dtype == CTWS_F32 ? 4 : 8;
    const int64_t N = nz * ny * nx, M = oz * oy * ox;
    const void* din;
    void* dout;
    if ((r = stage_in(h, h->ds_in, input, es * (size_t)N, dev, &din)) != CTWS_OK) return r;
    if ((r = out_begin(h, h->ds_out, out, es * (size_t)M, dev, &dout)) != CTWS_OK) return r;
    constexpr size_t kFlagBytes = sizeof(uint32_t) * kDsFlagSlots * kDsFlagStride;
    if ((r = grow(h, h->ds_flag, kFlagBytes)) != CTWS_OK) return r;
    DownscaleArgs a;
    a.in = din;
    a.out = dout;
    a.nz = (uint32_t)nz, a.ny = (uint32_t)ny, a.nx = (uint32_t)nx;
    a.oz = (uint32_t)oz, a.oy = (uint32_t)oy, a.ox = (uint32_t)ox;
    a.fz = (uint32_t)fz, a.fy = (uint32_t)fy, a.fx = (uint32_t)fx;
    a.flag = (uint32_t*)h->ds_flag.p;
    const int variant = (fy == 2 && fx == 2 && fz <= 2) ? (int)fz : 0;
    if (variant) {
        const int64_t C = 16 / (int64_t)es;  // output voxels per lane
        a.groups = (uint32_t)(nx / (2 * C));
        a.per = a.groups + ((int64_t)a.groups * C < ox ? 1u : 0u);
        a.items = (uint32_t)(oz * oy * (int64_t)a.per);  // (<= N)
    } else {
        a.groups = 0;
        a.per = (uint32_t)ox;
        a.items = (uint32_t)M;
    }
    const DsKernel k = dtype == CTWS_U8 ? ds_kernel<uint8_t>(func, variant)
                       : dtype == CTWS_U16 ? ds_kernel<uint16_t>(func, variant)
                       : dtype == CTWS_F32 ? ds_kernel<float>(func, variant)
                                           : ds_kernel<double>(func, variant);
    record(h, 0);
    HIPCHK(hipMemsetAsync(a.flag, 0, kFlagBytes, h->stream));
    k<<<(a.items + 255u) / 256u, 256, 0, h->stream>>>(a);
    LAUNCHCHK();
    record(h, 1);
    h->ds_flags.resize((size_t)kDsFlagSlots * kDsFlagStride);
    HIPCHK(hipMemcpyAsync(h->ds_flags.data(), a.flag, kFlagBytes, hipMemcpyDeviceToHost, h->stream));
    if ((r = out_end(h, out, dout, es * (size_t)M, dev)) != CTWS_OK) return r;
    uint32_t flag = 0;
    for (int k = 0; k < kDsFlagSlots; ++k) flag |= h->ds_flags[(size_t)k * kDsFlagStride];
    *any_nonzero = flag ? 1 : 0;
    stage_time(h, "downscale", 0, 1);
    return CTWS_OK;
}
}  // namespace

extern "C" {

int ctws_downscale_block(ctws_handle* h, const void* input, int dtype, int64_t nz, int64_t ny, int64_t nx,
                         const int64_t factors[3], int func, void* out, int64_t oz, int64_t oy, int64_t ox,
                         int* any_nonzero) {
    return downscale_block(h, input, dtype, nz, ny, nx, factors, func, out, oz, oy, ox, any_nonzero, false);
}

int ctws_downscale_block_device(ctws_handle* h, const void* input, int dtype, int64_t nz, int64_t ny, int64_t nx,
                                const int64_t factors[3], int func, void* out, int64_t oz, int64_t oy, int64_t ox,
                                int* any_nonzero) {
    return downscale_block(h, input, dtype, nz, ny, nx, factors, func, out, oz, oy, ox, any_nonzero, true);
}

}  // extern "C"
