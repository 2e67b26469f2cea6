// k_downscale.hip — DownscalingWorkflow on gfx950: one level of a scale pyramid by block reduction.
//
// Reference: downscaling/downscaling.py:222-229 and :309-310 with `library: 'skimage'`
// (`skimage.measure.block_reduce` of the float32 block, then clip, round, cast), restated in
// DESIGN.md section 3.9 and tests/downscaling_ref.py: every output voxel is the mean, maximum or
// minimum of its fz x fy x fx cell of the input, the input zero-padded at the end of every axis to a
// multiple of the factor (the zeros take part, the mean divides by fz fy fx).
//
//   value   uint8 / uint16 as integers, float32 as it is, float64 rounded to float32 first
//   mean    integers: the cell's sum in uint32 (exact, the entry point refuses n max >= 2^24),
//           float32(sum) / float32(n), rounded half to even, cast.  Floats: the sum in float64 in
//           the order z, y, x ascending, rounded once to float32, one float32 division.
//   max/min exact; a padded cell holds zeros.
// One pass, in + out bytes per call, no LDS and no floating-point atomic: an output voxel is a
// function of its cell, so repeated calls agree byte for byte.  The same pass takes the block's
// any-nonzero flag (`np.sum(x != 0) == 0`, -0.0 is zero): every input voxel is read exactly once.
//
//   k_downscale_vec<T, FUNC, FZ>  the pyramid's own factors (1, 2, 2) and (2, 2, 2).  A lane owns
//       16 bytes of an output row (C = 16 / sizeof(T) voxels): from each of the FZ * 2 input rows
//       it loads 32 bytes as two 16-byte loads, reduces pairs along x in registers, accumulates
//       the rows in registers and stores 16 bytes.  Rows start at any element (a pitch that is no
//       multiple of 16 bytes, nx = 67 with uint8): gfx950 under HSA takes dwordx4 accesses at any
//       address, so a row needs no scalar head.  Its tail -- the last nx % 2C input voxels and
//       the padded cell -- goes to one lane per output row through the scalar cell function.
//   k_downscale_cell<T, FUNC>     every other factor (1..8 each): a lane per output voxel, the
//       cell walked in z, y, x order with scalar loads; neighbouring lanes read neighbouring cells.
// Index arithmetic inside a block is 32-bit (a block holds fewer than 2^31 voxels).
#include "ctws_kernels.h"

namespace ctws {

namespace {

typedef uint32_t ds_u32x4 __attribute__((ext_vector_type(4)));

// a voxel as the reduction takes it
__device__ __forceinline__ uint32_t ds_value(uint8_t v) { return v; }
__device__ __forceinline__ uint32_t ds_value(uint16_t v) { return v; }
__device__ __forceinline__ float ds_value(float v) { return v; }
__device__ __forceinline__ float ds_value(double v) { return (float)v; }  // (round to nearest)

// the accumulator of one cell: integers
template <class T, int FUNC>
struct DsAcc {
    uint32_t a;
    __device__ __forceinline__ DsAcc() : a(FUNC == kDsMin ? 0xffffffffu : 0u) {}
    __device__ __forceinline__ void add(uint32_t v) {
        if (FUNC == kDsMean) a += v;
        else if (FUNC == kDsMax) a = v > a ? v : a;
        else a = v < a ? v : a;
    }
    __device__ __forceinline__ T finish(float n) const {
        if (FUNC != kDsMean) return (T)a;
        // the sum is below 2^24: the conversion is exact, the quotient lies in [0, max]
        return (T)__builtin_rintf(__fdiv_rn((float)a, n));
    }
};

// floats: the sum in float64, maximum and minimum in float32
template <class T, int FUNC>
struct DsAccF {
    double s;
    float m;
    __device__ __forceinline__ DsAccF()
        : s(0.0), m(FUNC == kDsMin ? __builtin_inff() : -__builtin_inff()) {}
    __device__ __forceinline__ void add(float v) {
        if (FUNC == kDsMean) s += (double)v;
        else if (FUNC == kDsMax) m = v > m ? v : m;
        else m = v < m ? v : m;
    }
    __device__ __forceinline__ T finish(float n) const {
        if (FUNC != kDsMean) return (T)m;
        return (T)__fdiv_rn((float)s, n);
    }
};
template <int FUNC>
struct DsAcc<float, FUNC> : DsAccF<float, FUNC> {};
template <int FUNC>
struct DsAcc<double, FUNC> : DsAccF<double, FUNC> {};

// one output voxel by scalar loads: the cell at (z0, y0, x0) of extent (fz, fy, fx), voxels past
// the block's end are zeros
template <class T, int FUNC>
__device__ __forceinline__ T ds_cell(const T* __restrict__ in, uint32_t nz, uint32_t ny, uint32_t nx, uint32_t z0,
                                     uint32_t y0, uint32_t x0, uint32_t fz, uint32_t fy, uint32_t fx, bool& any) {
    DsAcc<T, FUNC> acc;
    for (uint32_t dz = 0; dz < fz; ++dz) {
        for (uint32_t dy = 0; dy < fy; ++dy) {
            const uint32_t z = z0 + dz, y = y0 + dy;
            const bool row = z < nz && y < ny;
            const uint32_t rb = row ? (z * ny + y) * nx : 0u;
            for (uint32_t dx = 0; dx < fx; ++dx) {
                const uint32_t x = x0 + dx;
                T v = (T)0;
                if (row && x < nx) v = in[rb + x];
                any |= v != (T)0;
                acc.add(ds_value(v));
            }
        }
    }
    return acc.finish((float)(fz * fy * fx));
}

// a wave that saw a nonzero voxel sets its workgroup's slot of the flag table.  One word for the
// whole grid serialises in L2: an atomicOr per wave on it took 12 ns each, 0.2 ms for the 16,384
// waves of a float32 64 x 512 x 512 block (ten times the stream), a relaxed store 35 ns each.
// kDsFlagSlots words a cache line apart divide that by kDsFlagSlots; the host ORs them.
__device__ __forceinline__ void ds_flag(bool any, uint32_t* __restrict__ flag) {
    if (__ballot(any) != 0ull && (threadIdx.x & 63u) == 0u)
        atomicOr(flag + (blockIdx.x & (uint32_t)(kDsFlagSlots - 1)) * (uint32_t)kDsFlagStride, 1u);
}

}  // namespace

template <class T, int FUNC>
__global__ void __launch_bounds__(256) k_downscale_cell(DownscaleArgs a) {
    const T* __restrict__ in = (const T*)a.in;
    T* __restrict__ out = (T*)a.out;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool any = false;
    if (i < a.items) {  // items = oz * oy * ox
        const uint32_t orow = i / a.ox, x = i - orow * a.ox;
        const uint32_t z = orow / a.oy, y = orow - z * a.oy;
        out[i] = ds_cell<T, FUNC>(in, a.nz, a.ny, a.nx, z * a.fz, y * a.fy, x * a.fx, a.fz, a.fy, a.fx, any);
    }
    ds_flag(any, a.flag);
}

template <class T, int FUNC, int FZ>
__global__ void __launch_bounds__(256) k_downscale_vec(DownscaleArgs a) {
    constexpr uint32_t C = 16u / sizeof(T);  // output voxels per lane; 2C input voxels per row
    const T* __restrict__ in = (const T*)a.in;
    T* __restrict__ out = (T*)a.out;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool any = false;
    if (i < a.items) {  // items = oz * oy * per, per = groups + (a tail ? 1 : 0)
        const uint32_t orow = i / a.per, g = i - orow * a.per;
        const uint32_t oz = orow / a.oy, oy = orow - oz * a.oy;
        if (g < a.groups) {  // (g + 1) * 2C <= nx: every load lies inside its row
            DsAcc<T, FUNC> acc[C];
#pragma unroll
            for (uint32_t dz = 0; dz < (uint32_t)FZ; ++dz) {
#pragma unroll
                for (uint32_t dy = 0; dy < 2u; ++dy) {
                    const uint32_t z = oz * FZ + dz, y = oy * 2u + dy;
                    T e[2 * C];
                    if (z < a.nz && y < a.ny) {
                        const T* p = in + ((z * a.ny + y) * a.nx + g * 2u * C);
                        ds_u32x4 q0, q1;
                        __builtin_memcpy(&q0, p, 16);
                        __builtin_memcpy(&q1, p + C, 16);
                        __builtin_memcpy(&e[0], &q0, 16);
                        __builtin_memcpy(&e[C], &q1, 16);
                    } else {
#pragma unroll
                        for (uint32_t k = 0; k < 2u * C; ++k) e[k] = (T)0;
                    }
#pragma unroll
                    for (uint32_t c = 0; c < C; ++c) {
                        any |= e[2 * c] != (T)0;
                        any |= e[2 * c + 1] != (T)0;
                        acc[c].add(ds_value(e[2 * c]));
                        acc[c].add(ds_value(e[2 * c + 1]));
                    }
                }
            }
            T r[C];
#pragma unroll
            for (uint32_t c = 0; c < C; ++c) r[c] = acc[c].finish((float)(FZ * 4));
            ds_u32x4 q;
            __builtin_memcpy(&q, r, 16);
            __builtin_memcpy(out + (orow * a.ox + g * C), &q, 16);  // (g + 1) * C <= nx / 2 <= ox
        } else {
            // the row's tail: the output voxels from groups * C on (fewer than C + 1)
            for (uint32_t x = a.groups * C; x < a.ox; ++x)
                out[orow * a.ox + x] =
                    ds_cell<T, FUNC>(in, a.nz, a.ny, a.nx, oz * FZ, oy * 2u, x * 2u, (uint32_t)FZ, 2u, 2u, any);
        }
    }
    ds_flag(any, a.flag);
}

#define CTWS_DS_INST(T)                                                  \
    template __global__ void k_downscale_cell<T, kDsMean>(DownscaleArgs); \
    template __global__ void k_downscale_cell<T, kDsMax>(DownscaleArgs);  \
    template __global__ void k_downscale_cell<T, kDsMin>(DownscaleArgs);  \
    template __global__ void k_downscale_vec<T, kDsMean, 1>(DownscaleArgs); \
    template __global__ void k_downscale_vec<T, kDsMax, 1>(DownscaleArgs);  \
    template __global__ void k_downscale_vec<T, kDsMin, 1>(DownscaleArgs);  \
    template __global__ void k_downscale_vec<T, kDsMean, 2>(DownscaleArgs); \
    template __global__ void k_downscale_vec<T, kDsMax, 2>(DownscaleArgs);  \
    template __global__ void k_downscale_vec<T, kDsMin, 2>(DownscaleArgs);
CTWS_DS_INST(uint8_t)
CTWS_DS_INST(uint16_t)
CTWS_DS_INST(float)
CTWS_DS_INST(double)
#undef CTWS_DS_INST

}  // namespace ctws
