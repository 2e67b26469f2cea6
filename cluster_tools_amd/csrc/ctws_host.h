// ctws_host.h — internal to libctws.so (not installed next to include/ctws.h): the handle, and what
// every host translation unit of the library shares.  ctws_api.cpp holds open / close and the
// watershed path; each feature's entry points have a ctws_<feature>.cpp of their own.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ctws.h"
#include "ctws_kernels.h"
#include "host_pool.h"

namespace ctws {

// A device buffer that grow() sizes.  It frees itself, so a DevBuf member of the handle (or of one
// of its HostSlots) is released by ctws_close's `delete h` without being named there.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
        return *this;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

// The watershed path's arrays (ensure_workspace in ctws_api.cpp; freed by name in ctws_close).
struct Workspace {
    int64_t cap_vox = 0, cap_words = 0, cap_chunks = 0, cap_slices = 0, cap_tiles = 0, cap_blocks = 0;
    float *fin = nullptr, *dt = nullptr, *A = nullptr, *Bf = nullptr, *sm = nullptr, *hm = nullptr;
    uint8_t* cls = nullptr;
    uint32_t *P = nullptr, *PF = nullptr, *lab = nullptr;
    uint64_t* key = nullptr;
    uint64_t* W = nullptr;
    uint32_t *Wp = nullptr, *csum = nullptr;
    uint32_t *smin = nullptr, *smax = nullptr, *sb = nullptr, *slmax = nullptr, *soff = nullptr, *surv = nullptr;
    uint32_t *act0 = nullptr, *act1 = nullptr, *lines0 = nullptr, *lines1 = nullptr;
    BlockDesc* desc = nullptr;
    BlockStat* stat = nullptr;
    uint32_t* counter = nullptr;
    double* taps = nullptr;  // [6][128]
    // pass 2 (two-pass watershed) relabel hash
    int64_t cap_hash = 0;
    uint64_t* hkey = nullptr;
    uint32_t* hpos = nullptr;
    uint32_t* p2err = nullptr;
    // frontier bitmaps of the descent flood
    int64_t cap_front = 0;
    uint64_t *front0 = nullptr, *front1 = nullptr, *fopen = nullptr;
    uint64_t* fplat = nullptr;   // plateau fill (k_plateau.hip): the plateau voxels
    uint64_t* fseed = nullptr;   // seed CC members (the seed forest's parents are written for members only)
    uint32_t* plev = nullptr;    // per block: the plateau height (0: none)
    uint32_t* fflags = nullptr;
    uint32_t *fchunk0 = nullptr, *fchunk1 = nullptr;  // per 64-word chunk: generation of its last change
    uint32_t *wl0 = nullptr, *wl1 = nullptr, *qgen = nullptr;  // chunk worklists, queued generation
    uint32_t* wlcnt = nullptr;  // worklist length per iteration
    int64_t cap_fstat = 0;
    uint32_t* fstat = nullptr;  // CTWS_TRACE statistics: open voxels, frontier visits per block
    uint32_t* sfacc = nullptr;  // k_sf_plan's sums, 4 per block
};

constexpr int kFrontierMaxIters = 256;   // then the tile flood takes over

}  // namespace ctws

struct ctws_handle {
    using DevBuf = ctws::DevBuf;
    using Workspace = ctws::Workspace;
    using BlockDesc = ctws::BlockDesc;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    Workspace ws;
    uint32_t* h_counter = nullptr;  // pinned
    double* h_taps = nullptr;       // pinned [6][128]
    std::vector<std::pair<const char*, float>> timings;
    std::vector<hipEvent_t> events;
    hipEvent_t fev[2] = {nullptr, nullptr};
    uint64_t flood_tiles = 0, flood_iters = 0, flood_lines = 0;
    // host-pointer staging
    DevBuf st_in, st_mask, st_init, st_out;
    // host-pointer path: two slots of pinned host staging + device staging, copy streams
    struct HostSlot {
        void* pin_in = nullptr;  // inputs | masks | initial seeds of a batch, packed
        size_t pin_in_bytes = 0;
        void* pin_out = nullptr;  // uint64 outputs of a batch
        size_t pin_out_bytes = 0;
        DevBuf d_in, d_out;
        hipEvent_t ev_h2d = nullptr, ev_comp = nullptr, ev_d2h = nullptr;
        hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;  // CTWS_TRACE: the batch's upload, timed
        std::vector<hipEvent_t> ev_blk;  // per block of the batch: its output downloaded
    } hslot[2];
    hipStream_t s_in = nullptr, s_out = nullptr;
    // the temporary storage of the device-wide primitives (k_prims.hip).  One for all features: a
    // handle has one stream and runs one call at a time, and no primitive's temporary outlives it
    DevBuf prim_tmp;
    // relabel (k_relabel.hip)
    DevBuf rl_lab, rl_bits, rl_cnt, rl_offs, rl_out, rl_keys, rl_vals, rl_red;
    DevBuf rl_sorted, rl_uniq, rl_counts;  // sort-based unique
    int64_t rl_ntable = 0;  // entries of the resident assignment table (rl_keys / rl_vals)
    // EDT: counters (64 B) + columns queued for the lower-envelope pass (k_edt_col_fh)
    DevBuf edt_fh;
    DevBuf xface;  // crop CC: the tiles' x columns (CcArgs::xface)
    DevBuf ptile;  // plateau CC: per-tile plateau flags (CcArgs::ptile)
    DevBuf edt_scratch;  // k_edt_real_line: per-thread parabola stacks
    // WatershedFromSeeds (k_seeded.hip): distinct seed values, sorted values, segment offsets, sort temp
    DevBuf fs_vals, fs_sorted, fs_off, fs_tmp;
    // SizeFilterWorkflow (k_sizefilter.hip): the resident discard set (sorted ids; a bitmap over
    // [ids[0], ids[n - 1]] when that range is small), the blocks' descriptors, facts and seeds
    // (labels with the discarded ids zeroed), host-pointer staging of labels / height maps / outputs
    DevBuf sf_ids, sf_bits, sf_desc, sf_stat, sf_seeds, sf_lab, sf_hm, sf_out;
    // GraphWorkflow (k_rag.hip): host-pointer staging of labels / pairs / weights, the sorted
    // endpoint table, the emitted node ids, pairs and weights, keys (then the unique keys), sorted keys and
    // weights, summed weights, unpacked edges, counters (append, runs, missing)
    DevBuf rg_lab, rg_tab, rg_nodes, rg_pairs, rg_w, rg_keys, rg_skeys, rg_sw, rg_sum, rg_out, rg_red;
    // EdgeFeaturesWorkflow (k_edgefeat.hip): host-pointer staging of labels / data / nodes / edges / rows,
    // the edge keys, the sample keys and their sorted copy, counters (append, missing, bad edges)
    DevBuf ef_lab, ef_data, ef_nodes, ef_edges, ef_out, ef_ekeys, ef_keys, ef_skeys, ef_red;
    // NodeLabelWorkflow (k_overlaps.hip): host-pointer staging of the second label array (the
    // fragments take rg_lab), the rows (m x 3); everything else is the graph path's
    DevBuf ov_lab, ov_rows;
    // MorphologyWorkflow (k_morph.hip): the rows (m x 11) of the host-pointer path; the labels,
    // records and sort buffers are the graph path's
    DevBuf mo_rows, mo_acc;  // + the per-id integer table of the segments split over several waves
    // RegionFeaturesWorkflow (k_regfeat.hip): host-pointer staging of the input map and the rows
    // (m x 3), the rows' run counts and their scan, the records' sums, the chunk table (n, sum);
    // the labels, keys and sort buffers are the graph path's
    DevBuf rf_data, rf_rows, rf_cnt, rf_off, rf_sums, rf_ctab;
    // DownscalingWorkflow (k_downscale.hip): host-pointer staging of the block and its reduction,
    // the any-nonzero flag table and its host copy
    DevBuf ds_in, ds_out, ds_flag;
    std::vector<uint32_t> ds_flags;
    // RegionCentersWorkflow (k_regcenter.hip): host-pointer staging of the labels, the objects and
    // the lists of the two paths, the keys, the centres and flags of a host caller, the two scratch
    // arrays of the larger boxes
    DevBuf rc_lab, rc_objs, rc_list, rc_keys, rc_cent, rc_found, rc_a, rc_b;
    // ImageFilter (k_imgfilter.hip): host-pointer staging of the block and the response, the
    // responses between the passes (two after the first pass, three after the second), the taps of
    // the call (three axes x orders 0 and n) and the min / max words
    DevBuf if_in, if_out, if_a, if_b, if_taps, if_mm;
    // LiftedFeaturesFromNodeLabelsWorkflow (k_lifted.hip): host-pointer staging of the edges, the labels
    // and the rows; the degrees (then the fill's cursors), the CSR rows and lists, the labelled
    // nodes, the waves' queues and bitmaps, the keys and their sorted copy, counters
    DevBuf lf_edges, lf_lab, lf_out, lf_deg, lf_row, lf_adj, lf_src, lf_queue, lf_bits, lf_keys, lf_skeys, lf_red;
    // graph components and graph watershed (k_graphpost.hip): host-pointer staging of the edges, the
    // weights, the node array and the result; the parents and their second copy, the offers (also
    // the flags of a numbering) and the scanned flags, the edges' ends in rank order, the sort's keys
    // and indices with their sorted copies, counters
    DevBuf gp_edges, gp_w, gp_in, gp_out, gp_parent, gp_next, gp_best, gp_num, gp_su, gp_sv, gp_keys, gp_skeys, gp_idx,
        gp_sidx, gp_red;
    std::vector<double> if_taps_host;  // what if_taps holds: a job's calls share their taps
    int64_t sf_n = 0;
    uint64_t sf_lo = 1, sf_hi = 0;
    bool sf_has_bits = false;
    // ThresholdedComponents (k_threshcc.hip): forest, root bitmap, chunk counts / offsets, word
    // offsets, min / max + any flag, host-pointer staging
    DevBuf tc_P, tc_bits, tc_cnt, tc_offs, tc_woff, tc_red, tc_in, tc_mask, tc_out, tc_raw, tc_tmp, tc_taps;
    // evaluation (k_eval.hip): gt / seg / pair hash tables with counts, state, sums, staging
    DevBuf ev_ka, ev_ca, ev_kb, ev_cb, ev_kp, ev_cp, ev_state, ev_out, ev_stage;
    int64_t ev_cap_a = 0, ev_cap_b = 0, ev_cap_p = 0;
    // test hooks
    int stop_after = 0;
    int trace = 0;       // CTWS_TRACE=1: per-round flood statistics on stderr
    int no_descent = 0;  // CTWS_NO_DESCENT=1: flood from the seeds alone (test hook)
    int seed_tilecc = 0;  // CTWS_SEED_TILECC=1: the seed CC by tiles (else k_seed_members / k_seed_union2)
    // CTWS_SEED_DENSE=1: k_seed_members / k_plateau_flag over every class byte instead of the walk
    // over k_localmax's equal bitmap (k_seed_members_eq / k_plateau_flag_eq)
    int seed_dense = 0;
    int no_fallback = 0; // CTWS_NO_FALLBACK=1: keep a failed descent result (debugging)
    // CTWS_FORCE_WIDE=1: every flood on the wide keys (k_flood, 32-bit d; tests).  wide_rerun:
    // run_batch is re-running blocks whose packed flood reported a saturated d (dsat)
    int force_wide = 0;
    int wide_rerun = 0;
    int sf_sparse = 1;  // CTWS_SF_SPARSE=0: the size filter's regrow initialisation scans every block
    int fuse_hist = 1;  // CTWS_FUSE_HIST=0: the first flood's check and the label histogram as two kernels
    int verify = 1;      // CTWS_VERIFY: 1 (default) check the flood fixpoint + fallback, 2 fail on a violation (tests), 0 off
    int prep_lds = 0;    // CTWS_PREP_LDS=1: LDS row kernel for the x pass at every row length (tests)
    int plateau_fill = 1;  // CTWS_PLATEAU_FILL=0: masked blocks' plateaus relaxed hop by hop (k_plateau.hip)
    int output_tile = 1;   // CTWS_OUTPUT_TILE=0: cropped blocks through the word-tiled k_output
    int gauss_w = 0;            // CTWS_GAUSS_W (8, 16, 32): x positions per sliding-window column tile
    int gauss_yx = 1;           // CTWS_GAUSS_YX=0: separate y and x passes instead of the fused tile kernel
    int words_per_wave = 32;    // CTWS_WORDS_PER_WAVE: words per wave of the word-tiled kernels
    // CTWS_D2H_WGS: workgroups of a device-to-host copy kernel; 0 (default): hipMemcpyAsync on the
    // SDMA engines.  r03 (uint32 downloads, config 3): the copy kernel's workgroups slowed the
    // concurrent compute from 94 to 140 ms per step (host-resident 7.69 vs 6.08 Gvoxel/s)
    int d2h_wgs = 0;
    int pack_threads = 6;       // CTWS_PACK_THREADS: threads packing inputs into pinned staging
    int unpack_threads = 9;     // CTWS_UNPACK_THREADS: threads widening downloads into the outputs
    std::unique_ptr<ctws_host::WorkerPool> pack_pool, unpack_pool;
    int h2d_mode = 0;           // CTWS_H2D_MODE: 0 a copy per block as packed, 1 one copy per batch, 2 pull kernel
    int h2d_wgs = 64;           // CTWS_H2D_WGS: workgroups of the pull kernel (mode 2)
    int host_ramp = 1;          // CTWS_HOST_RAMP=0: equal batches (no smaller first / last batches)
    int host_batch_blocks = 0;  // CTWS_HOST_BATCH_BLOCKS: cap on blocks per host-path batch (0: voxel cap)
    int64_t host_batch_voxels = (int64_t)256 << 20;  // CTWS_HOST_BATCH_VOXELS: smaller batches pipeline better
    int edt_wz = 0;  // CTWS_EDT_WZ: the same for the z pass alone (3-D DT)
    // CTWS_EDT_BITS=0: the x pass writes g2 per voxel for every batch (k_prep_edt_x_co / _reg and
    // k_edt_col) instead of the records of k_edt_col_bits
    int edt_bits = 1;
    int edt_w = 0;  // CTWS_EDT_W (8, 16, 32, 64): x positions per EDT column tile (0: by line length)
    // CTWS_FRONTIER_CHUNK2D / _3D "CWxCYxCZ": frontier chunk brick (words x rows x slices, 64 words).
    // 3-D batches with a mask: 1x32x2 was their default until round 5 (a masked region is one
    // flat plateau the flood crosses hop by hop, and wider bricks in y cut the launches: config 5
    // 104 -> 72 ms before the plateau fill); with the plateau fill and the alternating sweep
    // order 1x8x8 relaxes config 5 faster (39.6 -> 36.4 ms, 132 -> 101 launches per step)
    int fchunk2[3] = {1, 64, 1};
    int fchunk3[3] = {1, 8, 8};
    int fchunk3_masked[3] = {1, 8, 8};
    int fchunk3_env = 0;  // CTWS_FRONTIER_CHUNK3D given: used for every 3-D batch
    int fc_cur[3] = {1, 64, 1};  // the brick of the current batch (run_batch)
    int cur_max[3] = {0, 0, 0};  // largest outer block extents (Z, Y, X) of the current batch
    // CTWS_FRONTIER_GRID: workgroups of k_frontier (chunks in flight / 4).  1024 rather than 2048:
    // half the chunks in flight keep more of each chunk's lines in L2 between its local sweeps
    // (r04: config 3 relaxation 20.3 -> 18.5 ms per step; 512: 23.0 ms, too few waves)
    int frontier_grid = 1024;
    int frontier_dir = 1;    // CTWS_FRONTIER_DIR: local sweeps queue only the neighbours a change may lower
    int frontier_reps = 32;  // CTWS_FRONTIER_REPS: local sweeps per chunk and launch (r02 sweep: 4 -> 32 cut k_frontier 19%)
    int frontier_max_iters = ctws::kFrontierMaxIters;  // CTWS_FRONTIER_ITERS: then the tile flood finishes
    std::vector<BlockDesc> last_desc;
    // pass 2 (2-D): per block of the next run_batch, the slice offsets of its previous run (empty:
    // none); a block with a wrapped-id merge runs again until its offsets are self-consistent
    std::vector<std::vector<uint32_t>> p2_hints;
    DevBuf p2_hint_dev;
    int p2_depth = 0;
    std::vector<uint8_t> last_bare;  // run_batch: per block, an in-mask voxel got the bare offset
};

// both return from a function that has the handle as `h`
#define HIPCHK(expr)                                                                     \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) {                                                          \
            h->err = std::string(#expr) + ": " + hipGetErrorString(e_);                  \
            return CTWS_EHIP;                                                            \
        }                                                                                \
    } while (0)

#define LAUNCHCHK()                                                                      \
    do {                                                                                 \
        hipError_t e_ = hipGetLastError();                                               \
        if (e_ != hipSuccess) {                                                          \
            h->err = std::string("kernel launch: ") + hipGetErrorString(e_);             \
            return CTWS_EHIP;                                                            \
        }                                                                                \
    } while (0)

// The non-template functions below are defined in ctws_host.cpp (unique_sorted: ctws_relabel.cpp).
namespace ctws {

// b holds at least bytes afterwards (its contents are not kept).  May hipFree, which waits for
// the device: a call grows all it needs before its first launch.
int grow(ctws_handle* h, DevBuf& b, size_t bytes);
// event idx of the handle, recorded on its stream
void record(ctws_handle* h, size_t idx);
// timings of one ctws_ws_blocks call: summed over its batches (counts too)
void add_timing(ctws_handle* h, const char* name, float v);
// an entry that names something of the last batch (prep_kernel): replaced, not summed
void set_timing(ctws_handle* h, const char* name, float v);
// the stage between events a and b of this call, in ms
void stage_time(ctws_handle* h, const char* name, size_t a, size_t b);
// host <-> device copy in pieces of at most 1 GiB: larger copies are not given to the SDMA
// engines but run as a blit kernel that competes with the compute kernels for the CUs
hipError_t copy_pieces(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);
// vigra Kernel1D<double>::initGaussian(sigma, 1.0) (restated; taps for offsets -r..r)
std::vector<double> gaussian_taps(double sigma);
// np.unique(labels[, return_counts]) by radix sort + run-length encoding (k_prims.hip): any
// value range.  dl: device labels; out / counts: caller buffers (device or host), cap entries.
int unique_sorted(ctws_handle* h, const uint64_t* dl, int64_t n, int on_device, uint64_t* out, uint64_t* counts,
                  int64_t cap, int64_t* n_unique);

// ---- the scaffold of the feature block calls ---------------------------------------------------
// The words of a feature's counter block (rg_red; the edge features' own ef_red).  The appends of
// all waves meet in an append counter, so each of the two has a 128-B line (16 words) to itself.
enum RedWord : size_t {
    kRedEmit = 0,       // the append counter of a counted emit
    kRedPairRuns = 1,   // pairs_tail: the unique pairs ...
    kRedPairMiss = 2,   // ... and the endpoint values missing from the id table
    kRedNodes = 16,     // graph: the append counter of the node ids
    kRedVmax = 16,      // morphology, region features: the largest id
    kRedMissing = 16,   // edge features: the owned voxel pairs without an edge
    kRedBadEdges = 17,  // edge features: edges not sorted, not unique or off the nodes
    kRedRuns = 19,      // sort_by_id: the distinct ids
    kRedWords = 32
};

int call_begin(ctws_handle* h);

// the kernels index a block with 32 bits: every extent and product of extents stays below 2^31
int check_extent(ctws_handle* h, int64_t nz, int64_t ny, int64_t nx, const char* what, const char* unit,
                 const char* why);

// An input array of a call -> *d, the device pointer to read: the caller's own with dev, else its
// copy in b.
template <class T>
int stage_in(ctws_handle* h, DevBuf& b, const T* src, size_t bytes, bool dev, const T** d) {
    *d = src;
    if (dev) return CTWS_OK;
    const int r = grow(h, b, bytes);
    if (r != CTWS_OK) return r;
    HIPCHK(copy_pieces(b.p, src, bytes, hipMemcpyHostToDevice, h->stream));
    *d = (const T*)b.p;
    return CTWS_OK;
}

// A result array of a call.  out_begin -> *d, the device pointer to write: the caller's own with
// dev, else b.  out_end ends the call: the download for a host caller, and the one wait.
template <class T>
int out_begin(ctws_handle* h, DevBuf& b, T* dst, size_t bytes, bool dev, T** d) {
    *d = dst;
    if (dev) return CTWS_OK;
    const int r = grow(h, b, bytes);
    *d = (T*)b.p;
    return r;
}

int out_end(ctws_handle* h, void* dst, const void* d, size_t bytes, bool dev);

// The counted emit.  A kernel appends records to buffers and counts every append, also those that
// found no room.  First capacities that depend on the block alone (so a call behaves the same
// whatever the handle ran before); the pass is repeated once at the counted sizes when one did
// not fit.
struct EmitCap {
    RedWord word;            // the counter that ...
    unsigned long long cap;  // ... this capacity bounds
};
struct Emitted {
    unsigned long long w[kRedWords] = {0};  // the counters as read back
    int passes = 0;
};
unsigned long long first_cap(int64_t n, int64_t div);

// cnt: the counter block; its first nzero words are zeroed before a pass and nread read back after
// it.  launch() grows the record buffers to caps and launches; check(w) is the feature's own look
// at the counters of a pass.
template <class Launch, class Check>
int counted_emit(ctws_handle* h, const char* what, unsigned long long* cnt, size_t nzero, size_t nread, EmitCap* caps,
                 int ncaps, Launch launch, Check check, Emitted* e) {
    int r, attempt = 0;
    for (; attempt < 2; ++attempt) {
        HIPCHK(hipMemsetAsync(cnt, 0, nzero * sizeof(uint64_t), h->stream));
        if ((r = launch()) != CTWS_OK) return r;
        LAUNCHCHK();
        HIPCHK(hipMemcpyAsync(e->w, cnt, nread * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if ((r = check(e->w)) != CTWS_OK) return r;
        bool fit = true;
        for (int c = 0; c < ncaps; ++c) fit = fit && e->w[caps[c].word] <= caps[c].cap;
        if (fit) break;
        if (attempt == 1) {
            h->err = std::string(what) + ": the emit counts changed between two passes over the same input";
            return CTWS_EHIP;
        }
        for (int c = 0; c < ncaps; ++c) caps[c].cap = std::max(caps[c].cap, e->w[caps[c].word]);
    }
    e->passes = attempt + 1;
    return CTWS_OK;
}

// a check of counted_emit: at least lo runs and at most one per voxel, or no second pass helps
int runs_within(ctws_handle* h, const char* what, unsigned long long runs, int64_t lo, int64_t n);

// Sort by id and run-length encode: n (id, record) pairs on the device -> the pairs sorted by id
// (rg_skeys, rg_sw) and the distinct ids with their numbers of pairs (rg_keys, rg_sum).  vmax: the
// largest id, for the sort's bits; the ids become float64 columns, so 2^53 or more is refused.
// ev: the event recorded behind the two launches.  The counters are those of rg_red.
struct ById {
    uint64_t *sids, *srecs, *uniq, *counts;
    int64_t m;  // the distinct ids
};
int sort_by_id(ctws_handle* h, const char* what, const uint64_t* ids, const uint64_t* recs, int64_t n,
               unsigned long long vmax, size_t ev, ById* o);

}  // namespace ctws
