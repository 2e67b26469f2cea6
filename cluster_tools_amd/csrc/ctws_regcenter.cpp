// ctws_regcenter.cpp — host side of libctws.so: RegionCentersWorkflow.
#include "ctws_host.h"

using namespace ctws;

// ---- RegionCentersWorkflow: the voxel farthest from the border per object (k_regcenter.hip) ---
namespace {
// the larger boxes run in groups that share the two scratch arrays: voxels and objects per group
// (a box above the voxel budget is a group of its own; the object budget is the grid's y limit)
constexpr int64_t kRcGroupVox = 1ll << 28;
constexpr int64_t kRcGroupObjs = 32768;

// k_rc_col's tile width for a line of L voxels in a box nx wide: the power of two that covers nx,
// at most 64, halved until the tile fits the LDS; 0 when a single column does not
uint32_t rc_tile_width(int64_t L, int64_t nx) {
    int64_t W = 1;
    while (W < 64 && W < nx) W <<= 1;
    while (W > 1 && L * W > kRcColWords) W >>= 1;
    return L * W > kRcColWords ? 0u : (uint32_t)W;
}

int region_centers(ctws_handle* h, const uint64_t* labels, int64_t n_labels, int64_t k, const uint64_t* ids,
                   const int64_t* offsets, const int64_t* shapes, const int64_t* pitches, const double* resolution,
                   int64_t* centers, uint8_t* found, bool dev) {
    int r;
    if (!h) return CTWS_EINVAL;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    if (n_labels < 0 || k < 0 || !resolution || (n_labels > 0 && !labels) ||
        (k > 0 && (!ids || !offsets || !shapes || !pitches || !centers || !found))) {
        h->err = "region centers: bad arguments (a label buffer, k objects with ids, offsets, shapes and pitches, "
                 "a resolution, centres and flags)";
        return CTWS_EINVAL;
    }
    if (k >= (1ll << 31)) {
        h->err = "region centers: 2^31 or more objects in one call";
        return CTWS_EUNSUPPORTED;
    }
    int64_t res[3];
    for (int d = 0; d < 3; ++d) {
        const double v = resolution[d];
        if (!(v > 0.0) || !std::isfinite(v)) {
            h->err = "region centers: a resolution that is not a positive number";
            return CTWS_EINVAL;
        }
        if (v != std::floor(v) || v > 1024.0) {
            h->err = "region centers: the resolution (" + std::to_string(resolution[0]) + ", " +
                     std::to_string(resolution[1]) + ", " + std::to_string(resolution[2]) +
                     ") is not three integers of at most 2^10.  The squared distances are exact integers only for "
                     "integer resolutions; otherwise float64 roundings decide ties.  The centre does not change when "
                     "all three values are scaled by a common factor: give [0.04, 0.004, 0.004] as [10, 1, 1]";
            return CTWS_EUNSUPPORTED;
        }
        res[d] = (int64_t)v;
    }
    if (k == 0) return CTWS_OK;
    std::vector<RcObj> objs((size_t)k);
    std::vector<uint32_t> small, large;
    for (int64_t i = 0; i < k; ++i) {
        const int64_t* s = shapes + 3 * i;
        const int64_t pz = pitches[2 * i], py = pitches[2 * i + 1];
        RcObj& o = objs[(size_t)i];
        o = RcObj{ids[i], offsets[i], pz, py, 0u, 0u, 0u, 0u, 0u, 0ull};
        const std::string who = "region centers: object " + std::to_string(i) + " (id " + std::to_string(ids[i]) + ")";
        if (s[0] < 0 || s[1] < 0 || s[2] < 0) {
            h->err = who + ": a negative extent";
            return CTWS_EINVAL;
        }
        if (s[0] == 0 || s[1] == 0 || s[2] == 0) continue;  // an empty box: not found
        // sum_a (r_a n_a)^2 < 2^31: every r_a n_a is below 46341 first, so the squares cannot overflow
        int64_t d2max = 0;
        bool over = false;
        for (int d = 0; d < 3; ++d) {
            if (s[d] >= 46341 || res[d] * s[d] >= 46341) over = true;
            else d2max += (res[d] * s[d]) * (res[d] * s[d]);
        }
        if (over || d2max >= (1ll << 31)) {
            h->err = who + ": a box of " + std::to_string(s[0]) + " x " + std::to_string(s[1]) + " x " +
                     std::to_string(s[2]) + " voxels at this resolution reaches a squared distance of 2^31 or more "
                     "(the transform is 32-bit)";
            return CTWS_EUNSUPPORTED;
        }
        const int64_t nvox = s[0] * s[1] * s[2];  // (each extent < 46341: no overflow)
        if (nvox >= (1ll << 31)) {
            h->err = who + ": 2^31 or more voxels in the box (the kernels index a box with 32 bits)";
            return CTWS_EUNSUPPORTED;
        }
        const unsigned __int128 last = (unsigned __int128)(s[0] - 1) * (unsigned __int128)(pz < 0 ? 0 : pz) +
                                       (unsigned __int128)(s[1] - 1) * (unsigned __int128)(py < 0 ? 0 : py) +
                                       (unsigned __int128)s[2];
        if (offsets[i] < 0 || py < s[2] || pz < 0 ||
            (s[0] > 1 && (__int128)pz < (__int128)(s[1] - 1) * (__int128)py + (__int128)s[2]) ||
            offsets[i] > n_labels || last > (unsigned __int128)(n_labels - offsets[i])) {
            h->err = who + ": the box does not lie inside the label buffer (offset, pitches and extents)";
            return CTWS_EINVAL;
        }
        o.nz = (uint32_t)s[0];
        o.ny = (uint32_t)s[1];
        o.nx = (uint32_t)s[2];
        if (nvox <= kRcSmallVox) {
            small.push_back((uint32_t)i);
        } else {
            o.wy = rc_tile_width(s[1], s[2]);
            o.wz = rc_tile_width(s[0], s[2]);
            large.push_back((uint32_t)i);
        }
    }
    // the groups of the larger boxes and each box's place in the scratch arrays
    struct Group {
        size_t first, n;
        int64_t vox;
    };
    std::vector<Group> groups;
    int64_t scratch_vox = 0;
    for (size_t j = 0; j < large.size(); ++j) {
        RcObj& o = objs[large[j]];
        const int64_t nvox = (int64_t)o.nz * o.ny * o.nx;
        if (groups.empty() || groups.back().vox + nvox > kRcGroupVox || (int64_t)groups.back().n >= kRcGroupObjs)
            groups.push_back(Group{j, 0, 0});
        o.sbase = (uint64_t)groups.back().vox;
        groups.back().n += 1;
        groups.back().vox += nvox;
        scratch_vox = std::max(scratch_vox, groups.back().vox);
    }
    const uint64_t* dl = labels;
    if (n_labels > 0 && (r = stage_in(h, h->rc_lab, labels, sizeof(uint64_t) * (size_t)n_labels, dev, &dl)) != CTWS_OK)
        return r;
    const size_t ob = sizeof(RcObj) * (size_t)k, lb = sizeof(uint32_t) * (small.size() + large.size());
    if ((r = grow(h, h->rc_objs, ob)) != CTWS_OK) return r;
    if ((r = grow(h, h->rc_list, std::max<size_t>(lb, 4))) != CTWS_OK) return r;
    if ((r = grow(h, h->rc_keys, sizeof(uint64_t) * (size_t)k)) != CTWS_OK) return r;
    if ((r = grow(h, h->rc_a, sizeof(uint32_t) * (size_t)scratch_vox)) != CTWS_OK) return r;
    if ((r = grow(h, h->rc_b, sizeof(uint32_t) * (size_t)scratch_vox)) != CTWS_OK) return r;
    const RcObj* dobjs = (const RcObj*)h->rc_objs.p;
    const uint32_t* dsmall = (const uint32_t*)h->rc_list.p;
    const uint32_t* dlarge = dsmall + small.size();
    unsigned long long* keys = (unsigned long long*)h->rc_keys.p;
    uint32_t *ga = (uint32_t*)h->rc_a.p, *gb = (uint32_t*)h->rc_b.p;
    long long* dcent;
    uint8_t* dfound;
    const size_t cb = 3 * sizeof(int64_t) * (size_t)k, fb = (size_t)k;
    if ((r = out_begin(h, h->rc_cent, (long long*)centers, cb, dev, &dcent)) != CTWS_OK) return r;
    if ((r = out_begin(h, h->rc_found, found, fb, dev, &dfound)) != CTWS_OK) return r;
    // (the vectors live until the call's one wait in out_end)
    HIPCHK(hipMemcpyAsync(h->rc_objs.p, objs.data(), ob, hipMemcpyHostToDevice, h->stream));
    if (!small.empty())
        HIPCHK(hipMemcpyAsync((void*)dsmall, small.data(), sizeof(uint32_t) * small.size(), hipMemcpyHostToDevice,
                              h->stream));
    if (!large.empty())
        HIPCHK(hipMemcpyAsync((void*)dlarge, large.data(), sizeof(uint32_t) * large.size(), hipMemcpyHostToDevice,
                              h->stream));
    HIPCHK(hipMemsetAsync(keys, 0, sizeof(uint64_t) * (size_t)k, h->stream));
    const RcRes rr = {(uint32_t)(res[0] * res[0]), (uint32_t)(res[1] * res[1]), (uint32_t)(res[2] * res[2])};
    record(h, 0);
    if (!small.empty()) {  // one launch serves all small objects of the call
        k_rc_small<<<(unsigned)small.size(), kRcSmallThreads, 0, h->stream>>>(dl, dobjs, dsmall, rr, keys);
        LAUNCHCHK();
    }
    record(h, 1);
    for (const Group& g : groups) {
        // the widest object of the group sizes the grid's x; every kernel strides over its own work
        int64_t rows = 1, tiles_y = 1, tiles_z = 1, vox = 1;
        bool staged_y = false, direct_y = false, staged_z = false, direct_z = false;
        for (size_t j = g.first; j < g.first + g.n; ++j) {
            const RcObj& o = objs[large[j]];
            rows = std::max<int64_t>(rows, (int64_t)o.nz * o.ny);
            vox = std::max<int64_t>(vox, (int64_t)o.nz * o.ny * o.nx);
            if (o.wy) tiles_y = std::max<int64_t>(tiles_y, (int64_t)o.nz * ((o.nx + o.wy - 1) / o.wy));
            if (o.wz) tiles_z = std::max<int64_t>(tiles_z, (int64_t)o.ny * ((o.nx + o.wz - 1) / o.wz));
            (o.wy ? staged_y : direct_y) = true;
            (o.wz ? staged_z : direct_z) = true;
        }
        const int64_t gcap = g.n > 64 ? 64 : 1024;  // many boxes fill the chip by their number
        const unsigned gy = (unsigned)g.n;
        const uint32_t* gl = dlarge + g.first;
        const dim3 grows((unsigned)std::min<int64_t>((rows + 3) / 4, gcap), gy);
        const dim3 gty((unsigned)std::min<int64_t>(tiles_y, gcap), gy), gtz((unsigned)std::min<int64_t>(tiles_z, gcap), gy);
        const dim3 gdir((unsigned)std::min<int64_t>((vox + 255) / 256, gcap), gy);
        k_rc_rows<<<grows, 256, 0, h->stream>>>(dl, dobjs, gl, rr, ga);
        LAUNCHCHK();
        if (staged_y) k_rc_col<true><<<gty, 256, 0, h->stream>>>(dobjs, gl, 1, rr.y2, 0, ga, gb, keys);
        if (direct_y) k_rc_col<false><<<gdir, 256, 0, h->stream>>>(dobjs, gl, 1, rr.y2, 0, ga, gb, keys);
        LAUNCHCHK();
        if (staged_z) k_rc_col<true><<<gtz, 256, 0, h->stream>>>(dobjs, gl, 0, rr.z2, 1, gb, ga, keys);
        if (direct_z) k_rc_col<false><<<gdir, 256, 0, h->stream>>>(dobjs, gl, 0, rr.z2, 1, gb, ga, keys);
        LAUNCHCHK();
    }
    record(h, 2);
    k_rc_finish<<<(unsigned)std::min<int64_t>((k + 255) / 256, 1024), 256, 0, h->stream>>>(dobjs, (uint32_t)k, keys, dcent,
                                                                                          dfound);
    LAUNCHCHK();
    if (!dev) HIPCHK(copy_pieces(centers, dcent, cb, hipMemcpyDeviceToHost, h->stream));
    if ((r = out_end(h, found, dfound, fb, dev)) != CTWS_OK) return r;
    stage_time(h, "rc_small", 0, 1);
    stage_time(h, "rc_large", 1, 2);
    add_timing(h, "rc_small_objects", (float)small.size());  // (counts, as the flood's rounds)
    add_timing(h, "rc_large_objects", (float)large.size());
    add_timing(h, "rc_large_groups", (float)groups.size());
    return CTWS_OK;
}
}  // namespace

extern "C" {

int ctws_region_centers(ctws_handle* h, const uint64_t* labels, int64_t n_labels, int64_t k, const uint64_t* ids,
                        const int64_t* offsets, const int64_t* shapes, const int64_t* pitches,
                        const double resolution[3], int64_t* centers, uint8_t* found) {
    return region_centers(h, labels, n_labels, k, ids, offsets, shapes, pitches, resolution, centers, found, false);
}

int ctws_region_centers_device(ctws_handle* h, const uint64_t* labels, int64_t n_labels, int64_t k, const uint64_t* ids,
                               const int64_t* offsets, const int64_t* shapes, const int64_t* pitches,
                               const double resolution[3], int64_t* centers, uint8_t* found) {
    return region_centers(h, labels, n_labels, k, ids, offsets, shapes, pitches, resolution, centers, found, true);
}

}  // extern "C"
