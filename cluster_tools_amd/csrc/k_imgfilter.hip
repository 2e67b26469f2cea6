// k_imgfilter.hip — ImageFilter: vigra's Gaussian derivative filters of one block.
//
// Reference: features/image_filter.py:105-115 (_apply_filter: vu.normalize of the outer block,
// vu.apply_filter, the inner box written), utils/volume_utils.py:95-120.  vigra semantics restated
// as in k_gauss.hip (Kernel1D::initGaussianDerivative + convolveLine, BORDER_TREATMENT_REFLECT):
//   out[i] = float( sum_{p = i-r}^{i+r} k[i-p] * (double) in[reflect(p)] )
// accumulated in double over ascending p, separate multiply and add (-ffp-contract=off), float32
// between the axes, axes in the order z, y, x.  The taps come from the host (ctws_filter_taps).
//
// The gradient magnitude and the Laplacian need three separable responses (S = smoothing, D = the
// derivative taps): S_x S_y D_z, S_x D_y S_z, D_x S_y S_z.  Nine single-output passes and a combine
// would move 88 B per voxel; the passes here share their inputs and move 48 B:
//   k_if_col<T, 1, 2>  z: reads the input (normalized on the fly), writes D_z and S_z     4 +  8 B
//   k_if_col<f, 2, 3>  y: reads those two, writes S_y D_z, D_y S_z, S_y S_z                8 + 12 B
//   k_if_row<3>        x: reads those three, convolves, writes the magnitude or the sum   12 +  4 B
// gaussianSmoothing runs k_if_col<T, 1, 1>, k_if_col<f, 1, 1>, k_if_row<1> (24 B); apply_in_2d
// starts at the y pass (k_if_col<T, 1, 2>) and ends in k_if_row<2>.  Each output of a pass is the
// arithmetic of a single-output pass, so the bits are those of the composition.
//
// One tile scheme for every radius up to kIfMaxR, radii at run time: the tile's lines with their
// halo of rmax sit in LDS (reflected at staging, so the tap loops read plain LDS), a thread owns
// several outputs and walks the taps once for all of them (one tap load per tap, not per output).
#include "ctws_kernels.h"

namespace ctws {

namespace {
__device__ __forceinline__ int if_reflect(int p, int L) { return p < 0 ? -p : (p >= L ? 2 * (L - 1) - p : p); }

// vu.normalize on the fly: float32(x) - min, divided by fl(max - min) when that is positive
struct IfNorm {
    float vmin, range;
    int on;
    __device__ __forceinline__ float operator()(float v) const {
        if (!on) return v;
        float t = v - vmin;
        if (range > 0.0f) t = t / range;
        return t;
    }
};
__device__ __forceinline__ IfNorm if_norm(const IfArgs& a) {
    IfNorm n{0.0f, 0.0f, a.normalize};
    if (a.normalize) {
        n.vmin = unordf(a.mm[0]);
        n.range = unordf(a.mm[1]) - n.vmin;
    }
    return n;
}
}  // namespace

// min / max of float32(x) as ordered bits (integer atomics: the result does not depend on the order).
// 16-byte loads, four in flight per lane, when the block is 16-byte aligned; the tail is scalar.
template <class T>
__global__ void __launch_bounds__(256) k_if_minmax(const T* __restrict__ v, int64_t n, uint32_t* __restrict__ mm) {
    constexpr int V = 16 / (int)sizeof(T);
    struct alignas(16) Vec {
        T e[V];
    };
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    auto take = [&](const Vec& a) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const uint32_t u = ordf((float)a.e[k]);
            lo = min(lo, u);
            hi = max(hi, u);
        }
    };
    const int64_t nv = (reinterpret_cast<uintptr_t>(v) & 15) == 0 ? n / V : 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const Vec* vv = reinterpret_cast<const Vec*>(v);
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < nv; i += 4 * stride) {
        const Vec a = vv[i], b = vv[i + stride], c = vv[i + 2 * stride], d = vv[i + 3 * stride];
        take(a), take(b), take(c), take(d);
    }
    for (; i < nv; i += stride) take(vv[i]);
    for (i = nv * V + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const uint32_t u = ordf((float)v[i]);
        lo = min(lo, u);
        hi = max(hi, u);
    }
    lo = wg_reduce_u32(lo, OpMin());
    hi = wg_reduce_u32(hi, OpMax());
    if (threadIdx.x == 0) {
        atomicMin(&mm[0], lo);
        atomicMax(&mm[1], hi);
    }
}
template __global__ void k_if_minmax<uint8_t>(const uint8_t*, int64_t, uint32_t*);
template __global__ void k_if_minmax<uint16_t>(const uint16_t*, int64_t, uint32_t*);
template __global__ void k_if_minmax<float>(const float*, int64_t, uint32_t*);
template __global__ void k_if_minmax<double>(const double*, int64_t, uint32_t*);

// Column pass along z (axis 0) or y (axis 1).  Tile = kIfColTL outputs along the axis x kIfColW
// consecutive x (lane = x: coalesced rows, conflict-free LDS); LDS holds NIN windows of
// kIfColTL + 2 rmax rows.  Wave w owns the tile rows w, w + 4, ...
template <class T, int NIN, int NOUT>
__global__ void __launch_bounds__(256) k_if_col(IfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float if_lds[];
    constexpr int TL = kIfColTL, W = kIfColW, U = TL / 4;
    const int L = a.axis == 0 ? a.nz : a.ny;
    const int other = a.axis == 0 ? a.ny : a.nz;
    const int nxc = (a.nx + W - 1) / W, ntl = (L + TL - 1) / TL;
    int t = blockIdx.x;
    const int xc = t % nxc;
    t /= nxc;
    const int lc = t % ntl, o = t / ntl;
    if (o >= other) return;
    const int64_t lstride = a.axis == 0 ? (int64_t)a.ny * a.nx : a.nx;
    const int64_t obase = a.axis == 0 ? (int64_t)o * a.nx : (int64_t)o * a.ny * a.nx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = xc * W + lane;
    const bool ok = x < a.nx;
    const int rmax = a.rmax;
    const int p0 = lc * TL, p1 = min(L, p0 + TL);
    const int rows = p1 - p0 + 2 * rmax;      // staged rows: line positions p0 - rmax .. p1 + rmax - 1
    const int wstride = (TL + 2 * rmax) * W;  // floats per input window
    const IfNorm norm = if_norm(a);
#pragma unroll
    for (int s = 0; s < NIN; ++s) {
        gptr_t<T> src = gbl((const T*)a.in[s]) + obase + (ok ? x : 0);
        float* win = if_lds + s * wstride + lane;
        staged_loop<8>(
            wave, rows, 4, [&](int m) { return norm((float)src[if_reflect(p0 - rmax + m, L) * lstride]); },
            [&](int m, float v) { win[m * W] = v; });
    }
    __syncthreads();
    if (!ok) return;
    gptr_t<double> taps = gbl(a.taps);
#pragma unroll
    for (int q = 0; q < NOUT; ++q) {
        const int s = (NIN == 1 || q == 0) ? 0 : 1;
        const int r = a.rad[q];
        gptr_t<double> k = taps + a.tap[q];
        // output row p0 + wave + 4 u reads the window rows wave + 4 u + rmax - r + m, m = 0 .. 2 r
        const float* win = if_lds + s * wstride + (wave + rmax - r) * W + lane;
        double sum[U];
#pragma unroll
        for (int u = 0; u < U; ++u) sum[u] = 0.0;
        for (int m = 0, j = 2 * r; j >= 0; ++m, --j) {
            const double kk = k[j];
#pragma unroll
            for (int u = 0; u < U; ++u) sum[u] += kk * (double)win[(m + 4 * u) * W];
        }
        gwptr_t<float> dst = gblw(a.out[q]) + obase + x;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + wave + 4 * u;
            if (p < p1) dst[p * lstride] = (float)sum[u];
        }
    }
}

#define CTWS_IF_COL(T, NIN, NOUT) template __global__ void k_if_col<T, NIN, NOUT>(IfArgs);
CTWS_IF_COL(uint8_t, 1, 1)
CTWS_IF_COL(uint16_t, 1, 1)
CTWS_IF_COL(float, 1, 1)
CTWS_IF_COL(double, 1, 1)
CTWS_IF_COL(uint8_t, 1, 2)
CTWS_IF_COL(uint16_t, 1, 2)
CTWS_IF_COL(float, 1, 2)
CTWS_IF_COL(double, 1, 2)
CTWS_IF_COL(float, 2, 3)
#undef CTWS_IF_COL

// Row pass along x and the combination.  A workgroup takes 4 rows (a wave each) x kIfRowW
// outputs; LDS holds NIN windows of kIfRowW + 2 rmax floats per wave.  Lane l owns the outputs
// l, l + 64, l + 128, l + 192 of the segment (consecutive lanes, consecutive LDS words).
// The square root of a float through the correctly rounded double one: rounding a 53-bit square
// root to 24 bits gives the correctly rounded float (53 >= 2 * 24 + 2).
template <int NIN>
__global__ void __launch_bounds__(256) k_if_row(IfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float if_lds[];
    constexpr int TW = kIfRowW, U = TW / 64;
    const int nseg = (a.nx + TW - 1) / TW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sc = blockIdx.x % nseg;
    const int64_t row = (int64_t)(blockIdx.x / nseg) * 4 + wave;
    const int64_t nrows = (int64_t)a.nz * a.ny;
    const bool rowok = row < nrows;
    const int rmax = a.rmax;
    const int x0 = sc * TW, x1 = min(a.nx, x0 + TW);
    const int cols = x1 - x0 + 2 * rmax;
    const int wlen = TW + 2 * rmax;
    float* wbase = if_lds + wave * NIN * wlen;
    if (rowok) {
#pragma unroll
        for (int s = 0; s < NIN; ++s) {
            gptr_t<float> src = gbl((const float*)a.in[s]) + row * a.nx;
            float* win = wbase + s * wlen;
            staged_loop<8>(
                lane, cols, 64, [&](int m) { return src[if_reflect(x0 - rmax + m, a.nx)]; },
                [&](int m, float v) { win[m] = v; });
        }
    }
    __syncthreads();
    if (!rowok) return;
    gptr_t<double> taps = gbl(a.taps);
    float res[NIN][U];
#pragma unroll
    for (int s = 0; s < NIN; ++s) {
        const int r = a.rad[s];
        gptr_t<double> k = taps + a.tap[s];
        const float* win = wbase + s * wlen + (rmax - r) + lane;
        double sum[U];
#pragma unroll
        for (int u = 0; u < U; ++u) sum[u] = 0.0;
        for (int m = 0, j = 2 * r; j >= 0; ++m, --j) {
            const double kk = k[j];
#pragma unroll
            for (int u = 0; u < U; ++u) sum[u] += kk * (double)win[m + 64 * u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) res[s][u] = (float)sum[u];
    }
    gwptr_t<float> dst = gblw(a.out[0]) + row * a.nx;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int x = x0 + lane + 64 * u;
        if (x >= x1) continue;
        float v = res[0][u];
        if (a.combine == kIfGradMag) {
            v = v * v;
#pragma unroll
            for (int s = 1; s < NIN; ++s) {
                const float sq = res[s][u] * res[s][u];
                v = v + sq;
            }
            v = (float)__dsqrt_rn((double)v);
        } else if (a.combine == kIfLaplace) {
#pragma unroll
            for (int s = 1; s < NIN; ++s) v = v + res[s][u];
        }
        dst[x] = v;
    }
}
template __global__ void k_if_row<1>(IfArgs);
template __global__ void k_if_row<2>(IfArgs);
template __global__ void k_if_row<3>(IfArgs);

}  // namespace ctws
