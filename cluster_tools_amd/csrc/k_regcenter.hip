// k_regcenter.hip — RegionCentersWorkflow on gfx950: for every object of a call the voxel of its
// box that is farthest from the box's background, by an exact integer Euclidean distance transform.
//
// Reference: morphology/region_centers.py:106-133 (`distance_transform_edt(labels[box] == id,
// sampling=resolution)` + `np.argmax`), restated in DESIGN.md section 3.10: with integer
// resolutions r the squared distance d2(p) = min over the voxels b of the box with label != id of
// sum_a (r_a (p_a - b_a))^2 is an exact integer, 0 outside the object, and the centre is the first
// voxel in C order with the largest d2.  The transform is separable: g_x(p) = r_x^2 (distance to
// the nearest background voxel on p's row)^2, g_y(p) = min_q g_x(.., q, ..) + r_y^2 (p_y - q)^2,
// d2 likewise along z.  A line without background carries kRcInf, an infinite parabola that no
// later pass picks; when it survives all three passes the box holds no background and the centre
// is the box's last voxel (what scipy returns there: DESIGN.md).  Every finite value stays below
// 2^31 (the host refuses a box with sum_a (r_a n_a)^2 >= 2^31), so kRcInf = 2^32 - 1 is never
// reached by a sum and 32-bit arithmetic is exact.
//
//   k_rc_small   boxes of at most kRcSmallVox voxels: one workgroup per object, the whole transform
//                in LDS.  The mask, then three passes that ping-pong between two arrays; a thread
//                owns a voxel and searches along its line outwards (rc_search: radius r while
//                p2 r^2 < best, as k_edt_col), so neighbouring lanes read neighbouring words.  The
//                z pass does not store: it reduces the key d2 << 32 | ~index by max.
//   k_rc_rows    larger boxes, x pass: a wave per row walks it in words of 64 voxels, the nearest
//                background to the left by a ballot and the carried last position, then backwards
//                the same to the right.
//   k_rc_col     larger boxes, y and z pass: tiles of W consecutive x by the whole line, staged in
//                LDS (W chosen by the host so that the line fits), the same search; lines too long
//                for the LDS search in the HBM scratch directly (STAGE = false).  The z pass
//                reduces the key per workgroup and takes one integer atomicMax per workgroup.
//   k_rc_finish  key -> the local (z, y, x) and the found flag.
// The argmax is a max over 64-bit integer keys: the result depends on the inputs alone.
#include "ctws_kernels.h"

namespace ctws {

// out(p) = min over the line's q of at(q) + p2 (p - q)^2, at(q) = kRcInf: no parabola at q.  Exact:
// no candidate farther than sqrt(best / p2) can win.  rr = p2 r^2 advances by its differences.
template <class At>
__device__ __forceinline__ uint32_t rc_search(At at, int p, int L, uint32_t p2) {
    uint32_t best = at(p);
    const int rlim = max(p, L - 1 - p);  // no candidates beyond
    uint32_t rr = p2, st = 3u * p2;
    for (int r = 1; r <= rlim; ++r) {
        if (rr >= best) break;
        const uint32_t a = at(max(p - r, 0)), b = at(min(p + r, L - 1));
        const uint32_t m = min(p - r >= 0 ? a : kRcInf, p + r < L ? b : kRcInf);
        if (m != kRcInf) best = min(best, m + rr);
        rr += st;
        st += 2u * p2;
    }
    return best;
}

__device__ __forceinline__ unsigned long long rc_key(uint32_t d2, uint32_t index) {
    return ((unsigned long long)d2 << 32) | (unsigned long long)(~index);
}

// the largest key of the workgroup (NW waves), valid in thread 0
template <int NW>
__device__ __forceinline__ unsigned long long rc_wg_max(unsigned long long key, unsigned long long* sh) {
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)key, s);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < NW; ++w) key = sh[w] > key ? sh[w] : key;
    return key;
}

__global__ void __launch_bounds__(kRcSmallThreads) k_rc_small(const uint64_t* __restrict__ lab,
                                                              const RcObj* __restrict__ objs,
                                                              const uint32_t* __restrict__ list, RcRes res,
                                                              unsigned long long* __restrict__ keys) {
    __shared__ uint32_t A[kRcSmallVox], B[kRcSmallVox];
    __shared__ unsigned long long wmax[kRcSmallThreads / 64];
    const uint32_t oi = list[blockIdx.x];
    const RcObj o = objs[oi];
    const int nx = (int)o.nx, ny = (int)o.ny, nz = (int)o.nz;
    const int yx = ny * nx, n = nz * yx;  // (n <= kRcSmallVox: the host's split)
    const uint64_t* __restrict__ src = lab + o.off;
    for (int i = threadIdx.x; i < n; i += kRcSmallThreads) {
        const int z = i / yx, rem = i - z * yx, y = rem / nx, x = rem - y * nx;
        A[i] = src[(int64_t)z * o.pz + (int64_t)y * o.py + x] == o.id ? kRcInf : 0u;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kRcSmallThreads) {
        const int row = i / nx, x = i - row * nx;
        const uint32_t* line = A + row * nx;
        B[i] = rc_search([&](int q) { return line[q]; }, x, nx, res.x2);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kRcSmallThreads) {
        const int z = i / yx, rem = i - z * yx, y = rem / nx, x = rem - y * nx;
        const uint32_t* line = B + z * yx + x;
        A[i] = rc_search([&](int q) { return line[q * nx]; }, y, ny, res.y2);
    }
    __syncthreads();
    unsigned long long key = 0ull;
    for (int i = threadIdx.x; i < n; i += kRcSmallThreads) {
        const int z = i / yx, rem = i - z * yx;
        const uint32_t* line = A + rem;
        const uint32_t d2 = rc_search([&](int q) { return line[q * yx]; }, z, nz, res.z2);
        const unsigned long long k = rc_key(d2, (uint32_t)i);
        key = k > key ? k : key;
    }
    key = rc_wg_max<kRcSmallThreads / 64>(key, wmax);
    if (threadIdx.x == 0) keys[oi] = key;
}

// x pass of the larger boxes: blockIdx.y = the object of the list, a wave per row
__global__ void __launch_bounds__(256) k_rc_rows(const uint64_t* __restrict__ lab, const RcObj* __restrict__ objs,
                                                 const uint32_t* __restrict__ list, RcRes res,
                                                 uint32_t* __restrict__ g) {
    const RcObj o = objs[list[blockIdx.y]];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const int nx = (int)o.nx;
    const uint32_t rows = o.nz * o.ny;
    const uint64_t le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);  // bits <= lane
    const uint64_t ge = ~0ull << lane;                                  // bits >= lane
    for (uint32_t r = wave0; r < rows; r += nwaves) {
        const uint32_t z = r / o.ny, y = r - z * o.ny;
        const uint64_t* __restrict__ src = lab + o.off + (int64_t)z * o.pz + (int64_t)y * o.py;
        uint32_t* __restrict__ dst = g + o.sbase + (uint64_t)r * (uint64_t)nx;
        // forwards: the distance to the nearest background at or before x
        int last = -1;
        for (int w0 = 0; w0 < nx; w0 += 64) {
            const int x = w0 + (int)lane;
            const bool in = x < nx;
            const uint64_t m = __ballot(in && src[in ? x : 0] != o.id);
            const uint64_t ml = m & le;
            const int left = ml ? w0 + 63 - __builtin_clzll(ml) : last;
            if (in) dst[x] = left < 0 ? kRcInf : (uint32_t)(x - left);
            if (m) last = w0 + 63 - __builtin_clzll(m);
        }
        // backwards: the nearer of that and the nearest background at or after x
        int first = -1;
        for (int w0 = ((nx - 1) >> 6) << 6; w0 >= 0; w0 -= 64) {
            const int x = w0 + (int)lane;
            const bool in = x < nx;
            const uint64_t m = __ballot(in && src[in ? x : 0] != o.id);
            const uint64_t mr = m & ge;
            const int right = mr ? w0 + __builtin_ctzll(mr) : first;
            if (in) {
                const uint32_t d = min(dst[x], right < 0 ? kRcInf : (uint32_t)(right - x));
                dst[x] = d == kRcInf ? kRcInf : res.x2 * d * d;
            }
            if (m) first = w0 + __builtin_ctzll(m);
        }
    }
}

// y (axis 1) or z (axis 0) pass of the larger boxes: blockIdx.y = the object of the list.  STAGE:
// the objects whose line fits the LDS at their tile width (RcObj::wy / wz > 0), else the others.
// final: no store, the key's maximum into keys[object].
template <bool STAGE>
__global__ void __launch_bounds__(256) k_rc_col(const RcObj* __restrict__ objs, const uint32_t* __restrict__ list,
                                                int axis, uint32_t p2, int final_pass,
                                                const uint32_t* __restrict__ gin, uint32_t* __restrict__ gout,
                                                unsigned long long* __restrict__ keys) {
    __shared__ uint32_t col[STAGE ? kRcColWords : 1];
    __shared__ unsigned long long wmax[4];
    const uint32_t oi = list[blockIdx.y];
    const RcObj o = objs[oi];
    const int W = (int)(axis == 1 ? o.wy : o.wz);
    if ((W > 0) != STAGE) return;
    const int nx = (int)o.nx, ny = (int)o.ny, nz = (int)o.nz;
    const int yx = ny * nx;
    const int L = axis == 1 ? ny : nz;
    const int other = axis == 1 ? nz : ny;  // the line index that is not x
    const int lstride = axis == 1 ? nx : yx;
    const int ostride = axis == 1 ? yx : nx;
    const uint32_t* __restrict__ src = gin + o.sbase;
    uint32_t* __restrict__ dst = gout + o.sbase;
    unsigned long long key = 0ull;
    if (STAGE) {
        const int nxc = (nx + W - 1) / W;
        const int c = threadIdx.x % W, r0 = threadIdx.x / W, RS = 256 / W;
        for (int t = blockIdx.x; t < other * nxc; t += gridDim.x) {
            const int ol = t / nxc, xb = (t - ol * nxc) * W;
            const bool colok = xb + c < nx;
            const int base = ol * ostride + xb + c;  // voxel (line position 0) of this thread's column
            for (int p = r0; p < L; p += RS) col[p * W + c] = colok ? src[base + p * lstride] : kRcInf;
            __syncthreads();
            if (colok)
                for (int p = r0; p < L; p += RS) {
                    const uint32_t d2 = rc_search([&](int q) { return col[q * W + c]; }, p, L, p2);
                    const int i = base + p * lstride;
                    if (final_pass) {
                        const unsigned long long k = rc_key(d2, (uint32_t)i);
                        key = k > key ? k : key;
                    } else {
                        dst[i] = d2;
                    }
                }
            __syncthreads();  // the next tile replaces the columns
        }
    } else {
        const int n = nz * yx;
        for (int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x; i64 < n; i64 += (int64_t)gridDim.x * 256) {
            const int i = (int)i64;
            const int z = i / yx, rem = i - z * yx, y = rem / nx;
            const int p = axis == 1 ? y : z;
            const uint32_t* line = src + (i - p * lstride);
            const uint32_t d2 = rc_search([&](int q) { return line[(int64_t)q * lstride]; }, p, L, p2);
            if (final_pass) {
                const unsigned long long k = rc_key(d2, (uint32_t)i);
                key = k > key ? k : key;
            } else {
                dst[i] = d2;
            }
        }
    }
    if (final_pass) {
        key = rc_wg_max<4>(key, wmax);
        if (threadIdx.x == 0 && key) atomicMax(keys + oi, key);
    }
}
template __global__ void k_rc_col<true>(const RcObj*, const uint32_t*, int, uint32_t, int, const uint32_t*, uint32_t*,
                                        unsigned long long*);
template __global__ void k_rc_col<false>(const RcObj*, const uint32_t*, int, uint32_t, int, const uint32_t*, uint32_t*,
                                         unsigned long long*);

// keys -> centres (k x 3, local) and found.  d2 = 0 (an empty box keeps its zeroed key; without a
// voxel of the id d2 is 0 everywhere) is not found; d2 = kRcInf: no background in the box, the
// centre is its last voxel.
__global__ void __launch_bounds__(256) k_rc_finish(const RcObj* __restrict__ objs, uint32_t k,
                                                   const unsigned long long* __restrict__ keys,
                                                   long long* __restrict__ centers, uint8_t* __restrict__ found) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < k; i += gridDim.x * blockDim.x) {
        const unsigned long long key = keys[i];
        const uint32_t d2 = (uint32_t)(key >> 32), idx = ~(uint32_t)key;
        long long z = 0, y = 0, x = 0;
        if (d2 == kRcInf) {
            z = (long long)objs[i].nz - 1;
            y = (long long)objs[i].ny - 1;
            x = (long long)objs[i].nx - 1;
        } else if (d2 != 0u) {
            const uint32_t nx = objs[i].nx, yx = objs[i].ny * nx;
            const uint32_t rem = idx % yx;
            z = idx / yx;
            y = rem / nx;
            x = rem % nx;
        }
        centers[3 * (size_t)i] = z;
        centers[3 * (size_t)i + 1] = y;
        centers[3 * (size_t)i + 2] = x;
        found[i] = d2 != 0u ? 1 : 0;
    }
}

}  // namespace ctws
