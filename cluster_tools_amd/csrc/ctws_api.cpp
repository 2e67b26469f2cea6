// ctws_api.cpp — host side of libctws.so: the C-ABI of include/ctws.h.
//
// Replaces the block loop of the reference job entry (cluster_tools/watershed/watershed.py:
// 380-381, `for block_id in block_list: _ws_block(...)`) with batched launches: all blocks of
// a batch go through one pipeline of gfx950 kernels (grid.y = block), so even a single job
// fills the 256 CUs.  The caller keeps the dataset I/O and the "processed block" log protocol.
//
// Pipeline per batch (kernel files in brackets):
//   input min/max -> normalize + threshold + EDT x  [k_edt]     (_read_data, _apply_dt)
//   EDT y [, z] -> dt, dt min/max                    [k_edt]
//   Gaussian(sigma_seeds) of dt                      [k_gauss]   (_make_seeds)
//   hmap + Gaussian(sigma_weights)                   [k_gauss]   (_make_hmap)
//   local maxima, plateaus, seed CC, scan-order ids  [k_cc]
//   seeded flood                                     [k_flood]   (watershedsNew)
//   size filter + regrow flood                       [k_post, k_flood] (apply_size_filter)
//   2-D slice offsets / mask                         [k_post]    (_apply_watershed)
//   halo crop CC + uint64 offset                     [k_cc]      (_ws_block :326-341)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <type_traits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <climits>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/ctws.h"
#include "ctws_kernels.h"
#include "host_pool.h"

using namespace ctws;

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

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

constexpr int kCounterBytes = 4 * (4 + 4 * kStatSlots);  // flood flag + statistics slots
constexpr int kFrontierBatch = 8;        // frontier iterations per host check
constexpr int kFrontierWavesHost = 4;    // waves per workgroup of k_frontier (kFrontierWaves)
constexpr int kFrontierMaxIters = 256;   // then the tile flood takes over
constexpr int kFrontierMaxItersCap = 4096;  // CTWS_FRONTIER_ITERS upper bound (worklist counters)

}  // namespace

struct ctws_handle {
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
    // relabel (k_relabel.hip)
    DevBuf rl_lab, rl_bits, rl_cnt, rl_offs, rl_out, rl_keys, rl_vals, rl_red;
    DevBuf rl_sorted, rl_uniq, rl_counts, rl_tmp;  // sort-based unique
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
    // weights, summed weights, unpacked edges, sort / reduce temp, counters (append, runs, missing)
    DevBuf rg_lab, rg_tab, rg_nodes, rg_pairs, rg_w, rg_keys, rg_skeys, rg_sw, rg_sum, rg_out, rg_tmp, rg_red;
    // EdgeFeaturesWorkflow (k_edgefeat.hip): host-pointer staging of labels / data / nodes / edges / rows,
    // the edge keys, the sample keys and their sorted copy, sort temp, counters (append, missing, bad edges)
    DevBuf ef_lab, ef_data, ef_nodes, ef_edges, ef_out, ef_ekeys, ef_keys, ef_skeys, ef_tmp, ef_red;
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
    // nodes, the waves' queues and bitmaps, the keys and their sorted copy, scan / sort temp, counters
    DevBuf lf_edges, lf_lab, lf_out, lf_deg, lf_row, lf_adj, lf_src, lf_queue, lf_bits, lf_keys, lf_skeys, lf_tmp, lf_red;
    // graph components and graph watershed (k_graphpost.hip): host-pointer staging of the edges, the
    // weights, the node array and the result; the parents and their second copy, the offers (also
    // the flags of a numbering) and the scanned flags, the edges' ends in rank order, the sort's keys
    // and indices with their sorted copies, scan / sort temp, counters
    DevBuf gp_edges, gp_w, gp_in, gp_out, gp_parent, gp_next, gp_best, gp_num, gp_su, gp_sv, gp_keys, gp_skeys, gp_idx,
        gp_sidx, gp_tmp, gp_red;
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
    int frontier_max_iters = kFrontierMaxIters;  // CTWS_FRONTIER_ITERS: then the tile flood finishes
    std::vector<BlockDesc> last_desc;
    // pass 2 (2-D): per block of the next run_batch, the slice offsets of its previous run (empty:
    // none); a block with a wrapped-id merge runs again until its offsets are self-consistent
    std::vector<std::vector<uint32_t>> p2_hints;
    DevBuf p2_hint_dev;
    int p2_depth = 0;
    std::vector<uint8_t> last_bare;  // run_batch: per block, an in-mask voxel got the bare offset
};

namespace {

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

template <class T>
int dev_alloc(ctws_handle* h, T*& p, int64_t n) {
    if (p) {
        hipFree(p);
        p = nullptr;
    }
    if (n <= 0) n = 1;
    hipError_t e = hipMalloc((void**)&p, sizeof(T) * (size_t)n);
    if (e != hipSuccess) {
        h->err = std::string("hipMalloc(") + std::to_string(sizeof(T) * (size_t)n) + "): " + hipGetErrorString(e);
        p = nullptr;
        return CTWS_ENOMEM;
    }
    return CTWS_OK;
}

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

int ensure_workspace(ctws_handle* h, int64_t vox, int64_t words, int64_t chunks, int64_t slices, int64_t tiles,
                     int64_t blocks, int64_t hash, int64_t front) {
    Workspace& w = h->ws;
    int r = CTWS_OK;
#define ALLOC(field, n) \
    if ((r = dev_alloc(h, w.field, (n))) != CTWS_OK) return r
    if (vox > w.cap_vox) {
        vox = std::max<int64_t>(vox, w.cap_vox + w.cap_vox / 4);
        ALLOC(fin, vox);
        ALLOC(dt, vox);
        ALLOC(A, vox);
        ALLOC(Bf, vox);
        ALLOC(sm, vox);
        ALLOC(hm, vox);
        ALLOC(cls, vox + 16);  // k_plateau_flag reads aligned 16-byte groups
        ALLOC(P, vox + 4);
        ALLOC(PF, vox + 4);
        ALLOC(lab, vox);
        ALLOC(key, vox);
        w.cap_vox = vox;
    }
    if (words > w.cap_words) {
        ALLOC(W, words);
        ALLOC(Wp, words);
        w.cap_words = words;
    }
    if (chunks > w.cap_chunks) {
        ALLOC(csum, chunks);
        w.cap_chunks = chunks;
    }
    if (slices > w.cap_slices) {
        ALLOC(smin, slices);
        ALLOC(smax, slices);
        ALLOC(sb, slices);
        ALLOC(slmax, slices);
        ALLOC(soff, slices);
        ALLOC(surv, slices);
        w.cap_slices = slices;
    }
    if (tiles > w.cap_tiles) {
        ALLOC(act0, tiles);
        ALLOC(act1, tiles);
        ALLOC(lines0, tiles * kLineWords);
        ALLOC(lines1, tiles * kLineWords);
        w.cap_tiles = tiles;
    }
    if (blocks > w.cap_blocks) {
        ALLOC(desc, blocks);
        ALLOC(stat, blocks);
        w.cap_blocks = blocks;
    }
    if (hash > w.cap_hash) {
        ALLOC(hkey, hash);
        ALLOC(hpos, hash);
        w.cap_hash = hash;
    }
    if (!w.p2err) ALLOC(p2err, 4);
    if (front > w.cap_front) {
        ALLOC(front0, front);
        ALLOC(front1, front);
        ALLOC(fopen, front);
        ALLOC(fplat, front);
        ALLOC(fseed, front);
        ALLOC(fchunk0, (front >> kChunkShift) + 1);
        ALLOC(fchunk1, (front >> kChunkShift) + 1);
        ALLOC(wl0, (front >> kChunkShift) + 1);
        ALLOC(wl1, (front >> kChunkShift) + 1);
        ALLOC(qgen, (front >> kChunkShift) + 1);
        w.cap_front = front;
    }
    if (!w.fflags) ALLOC(fflags, kFrontierBatch);
    if (!w.wlcnt) ALLOC(wlcnt, kFrontierMaxItersCap + 2);
    if (blocks > w.cap_fstat) {
        ALLOC(fstat, 3 * blocks);
        ALLOC(plev, blocks);
        ALLOC(sfacc, 4 * blocks);
        HIPCHK(hipMemsetAsync(w.sfacc, 0, sizeof(uint32_t) * 4 * (size_t)blocks, h->stream));  // (k_sf_plan keeps it zero)
        w.cap_fstat = blocks;
    }
    if (!w.counter) ALLOC(counter, kCounterBytes / 4);
    if (!w.taps) ALLOC(taps, 6 * kTapSlot);
#undef ALLOC
    return CTWS_OK;
}

// vigra Kernel1D<double>::initGaussian(sigma, 1.0) (restated; taps for offsets -r..r)
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

struct BlockIO {
    const void* in;
    const uint8_t* mask;
    const uint64_t* init;
    uint64_t* out;
    uint32_t* out32 = nullptr;  // host path: compact uint32 codes (widened on the host)
};

struct Plan {
    // validated, derived configuration
    int nd_ws, dt_2d, pass2;
    int from_seeds;  // WatershedFromSeeds (watershed_from_seeds.py): given seeds, hmap = input
    // the filling size filter (postprocess/filling_size_filter.py) on the from_seeds plan: the
    // hmap is the RAW input cast to float32 (no normalize) and the seeds keep their uint64 values
    int sf_fill;
    int pitch[3];
    double pitchd[3];  // pixel_pitch as given
    bool real_pitch;   // a non-integer pitch: vigra's double-temporary distance path
    bool seeds_smooth, weights_smooth;
    double sig_seeds[3], sig_weights[3];
};

int make_plan(ctws_handle* h, const ctws_cfg* cfg, Plan& p) {
    p.from_seeds = 0;
    p.sf_fill = 0;
    p.nd_ws = cfg->apply_ws_2d ? 2 : 3;
    p.dt_2d = cfg->apply_dt_2d ? 1 : 0;
    if (cfg->pass_id != 0 && cfg->pass_id != 1) {
        h->err = "pass_id must be 0 (_ws_block) or 1 (_ws_pass2)";
        return CTWS_EINVAL;
    }
    p.pass2 = cfg->pass_id == 1 ? 1 : 0;
    for (int k = 0; k < 3; ++k) {
        p.pitch[k] = 1;
        p.pitchd[k] = 1.0;
    }
    p.real_pitch = false;
    if (cfg->has_pixel_pitch) {
        if (p.dt_2d) {
            h->err = "apply_dt_2d requires pixel_pitch None (watershed.py:151)";
            return CTWS_EINVAL;
        }
        for (int k = 0; k < 3; ++k) {
            const double v = cfg->pixel_pitch[k];
            if (!(v > 0.0) || !std::isfinite(v)) {
                h->err = "pixel_pitch must be positive";
                return CTWS_EINVAL;
            }
            p.pitchd[k] = v;
            // vigra: int(pitch) != pitch selects the real-valued (double) path (multi_distance.hxx);
            // a large integer pitch stays integer: its dmax >= 2^24 selects the float path per batch
            // (run_batch), as the oracle's distance_transform does.  (The int copy is only read by
            // the exact integer path, which such a pitch never takes.)
            if (v != std::floor(v)) p.real_pitch = true;
            else p.pitch[k] = (int)std::min(v, 65536.0);
        }
    }
    auto sig = [&](const double* s, int is_list, double* out, bool& en) -> int {
        en = is_list ? true : (s[0] != 0.0);
        if (is_list && p.nd_ws == 2) {
            h->err = "per-axis sigma needs a 3-D watershed (volume_utils.py:97-98)";
            return CTWS_EINVAL;
        }
        for (int k = 0; k < 3; ++k) {
            out[k] = is_list ? s[k] : s[0];
            if (out[k] < 0.0) {
                h->err = "negative sigma";
                return CTWS_EINVAL;
            }
            if ((int)(3.0 * out[k] + 0.5) >= kTapSlot / 2) {
                h->err = "sigma too large (radius >= 2048)";
                return CTWS_EUNSUPPORTED;
            }
        }
        return CTWS_OK;
    };
    int r;
    if ((r = sig(cfg->sigma_seeds, cfg->sigma_seeds_is_list, p.sig_seeds, p.seeds_smooth)) != CTWS_OK) return r;
    if ((r = sig(cfg->sigma_weights, cfg->sigma_weights_is_list, p.sig_weights, p.weights_smooth)) != CTWS_OK)
        return r;
    return CTWS_OK;
}

int col_width(int L) { return L <= 512 ? 32 : (L <= 1024 ? 16 : 8); }

// dynamic LDS above 64 KiB needs the kernel's opt-in (gfx950: up to 160 KiB per workgroup)
constexpr size_t kMaxLds = 160 * 1024;
template <class K>
void lds_optin(K kern, size_t lds) {
    if (lds > 65536) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}
// The largest outer block extents the LDS line kernels take: a whole row in LDS (k_prep_edt_x:
// 16 B per voxel; k_gauss_row: 16 B per voxel + 1 KiB) and whole y / z columns 8 wide (k_edt_col<8>,
// k_gauss_col<8>: 32 B per position + 1 KiB).  Round 6: the former caps X <= 4096, Y, Z <= 2048
// were the 64 KiB default, not the hardware.
constexpr int kMaxRowX = (int)((kMaxLds - 1024) / 16);    // 10176
constexpr int kMaxColLen = (int)((kMaxLds - 1024) / 32);  // 5088
// EDT columns: 16 x positions (64-B row segments) beat 32 — half the LDS per tile, twice the
// tiles per CU, and the bounded search's per-lane trip counts vary less per wave (r01 sweep:
// y+z passes 1.60 ms at 32, 1.44 at 16, 1.77 at 8 for config 2)
// EDT column tile width: 32 x positions (full 128-B rows) while the column tile fits 32 KiB
// of LDS (config 4/5 z pass, 80-deep lines: 14.9 -> 13.8 / 14.3 -> 12.7 ms of EDT per step);
// 16 up to 1024-long lines (a 576-long y line at 32 wide, 74 KiB, measured 9.1 vs 5.6 ms)
int edt_col_width(int L) { return L <= 256 ? 32 : L <= 1024 ? 16 : 8; }

void record(ctws_handle* h, size_t idx) {
    while (h->events.size() <= idx) {
        hipEvent_t e;
        hipEventCreate(&e);
        h->events.push_back(e);
    }
    hipEventRecord(h->events[idx], h->stream);
}

// ---- Gaussian passes over the active axes, z -> y -> x --------------------------------------
#define CTWS_R12(M) M(1), M(2), M(3), M(4), M(5), M(6), M(7), M(8), M(9), M(10), M(11), M(12)
#define CTWS_ROWR(R) &k_gauss_row_r<R>
#define CTWS_COL32(R) &k_gauss_col_r<32, R>
#define CTWS_COL16(R) &k_gauss_col_r<16, R>
#define CTWS_COL8(R) &k_gauss_col_r<8, R>
using GaussKernel = decltype(&k_gauss_row_r<1>);
const GaussKernel kGaussRowR[kGaussMaxR + 1] = {nullptr, CTWS_R12(CTWS_ROWR)};
const GaussKernel kGaussColR32[kGaussMaxR + 1] = {nullptr, CTWS_R12(CTWS_COL32)};
const GaussKernel kGaussColR16[kGaussMaxR + 1] = {nullptr, CTWS_R12(CTWS_COL16)};
const GaussKernel kGaussColR8[kGaussMaxR + 1] = {nullptr, CTWS_R12(CTWS_COL8)};
#define CTWS_YX(R) &k_gauss_yx<R>
using GaussYxKernel = decltype(&k_gauss_yx<1>);
const GaussYxKernel kGaussYx[kGaussMaxR + 1] = {nullptr, CTWS_R12(CTWS_YX)};
#undef CTWS_YX
#undef CTWS_R12
#undef CTWS_ROWR
#undef CTWS_COL32
#undef CTWS_COL16
#undef CTWS_COL8

int run_gauss(ctws_handle* h, const Plan& pl, const double* sig, bool hmap_src, const float* src, float* dst,
              int nb, int maxZ, int maxY, int maxX, HmapParams hp, int taps_slot) {
    Workspace& w = h->ws;
    int axes[3], na = 0;
    for (int a = (pl.nd_ws == 3 ? 0 : 1); a < 3; ++a)
        if (sig[a] > 0.0) axes[na++] = a;
    if (na == 0) {
        if (hmap_src) {
            dim3 g((unsigned)std::min<int64_t>(((int64_t)maxZ * maxY * maxX + 255) / 256, 4096), nb);
            k_hmap<<<g, 256, 0, h->stream>>>(w.desc, w.stat, hp, w.fin, w.dt, w.smin, w.smax, dst);
            LAUNCHCHK();
        } else if (src != dst) {
            // identity smoothing: the caller reads `src`
        }
        return CTWS_OK;
    }
    const float* cur = src;
    for (int i = 0; i < na; ++i) {
        const int a = axes[i];
        auto taps = gaussian_taps(sig[a]);
        const int r = (int)taps.size() / 2;
        double* dtaps = w.taps + (taps_slot * 3 + a) * kTapSlot;
        double* htaps = h->h_taps + (taps_slot * 3 + a) * kTapSlot;
        std::memcpy(htaps, taps.data(), sizeof(double) * taps.size());
        HIPCHK(hipMemcpyAsync(dtaps, htaps, sizeof(double) * taps.size(), hipMemcpyHostToDevice, h->stream));
        float* out = (i == na - 1) ? dst : ((i % 2 == 0) ? w.A : w.Bf);
        GaussParams gp{a, r, (i == 0 && hmap_src) ? 1 : 0};
        const float* in = (i == 0 && hmap_src) ? w.fin : cur;
        // the last two axes y, x with one radius: fused tile kernel (k_gauss_yx)
        if (h->gauss_yx && a == 1 && i + 1 == na - 1 && axes[i + 1] == 2 && r >= 1 && r <= kGaussMaxR) {
            auto tx = gaussian_taps(sig[2]);
            if ((int)tx.size() / 2 == r) {
                double* dtx = w.taps + (taps_slot * 3 + 2) * kTapSlot;
                double* htx = h->h_taps + (taps_slot * 3 + 2) * kTapSlot;
                std::memcpy(htx, tx.data(), sizeof(double) * tx.size());
                HIPCHK(hipMemcpyAsync(dtx, htx, sizeof(double) * tx.size(), hipMemcpyHostToDevice, h->stream));
                const int TX = 128 - 2 * r;
                const int64_t ntiles = (int64_t)maxZ * ((maxY + kGaussYxTY - 1) / kGaussYxTY) * ((maxX + TX - 1) / TX);
                dim3 g((unsigned)ntiles, nb);
                hipLaunchKernelGGL(kGaussYx[r], g, dim3(256), 0, h->stream, w.desc, w.stat, gp.hmap_src, hp,
                                   (const double*)dtaps, (const double*)dtx, in, (const float*)w.dt,
                                   (const uint32_t*)w.smin, (const uint32_t*)w.smax, dst);
                LAUNCHCHK();
                return CTWS_OK;
            }
        }
        if (r >= 1 && r <= kGaussMaxR) {
            // sliding-window kernels (k_gauss.hip)
            if (a == 2 && maxX > 1024) {
                // rows longer than a wave's registers hold: the generic row kernel
                dim3 g((unsigned)(((int64_t)maxZ * maxY + 3) / 4), nb);
                const size_t lds = 2 * 128 * 4 + 4 * (size_t)maxX * 4;
                if (lds > 65536)  // gfx950: up to 160 KiB of LDS per workgroup, above 64 KiB by opt-in
                    (void)hipFuncSetAttribute((const void*)k_gauss_row, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)lds);
                k_gauss_row<<<g, 256, lds, h->stream>>>(w.desc, w.stat, gp, hp, dtaps, in, w.dt, w.smin, w.smax, out);
            } else if (a == 2) {
                // rows per wave shrink with X: size the grid for the widest block
                const int rpw = 64 / ((maxX + 15) / 16);
                dim3 g((unsigned)(((int64_t)maxZ * maxY + 4 * rpw - 1) / (4 * rpw)), nb);
                const size_t lds = 4 * 2 * (size_t)(64 * 17 + 64) * 4;
                hipLaunchKernelGGL(kGaussRowR[r], g, dim3(256), lds, h->stream, w.desc, w.stat, gp, hp,
                                   (const double*)dtaps, in, (const float*)w.dt, (const uint32_t*)w.smin,
                                   (const uint32_t*)w.smax, out);
            } else {
                const int Lm = a == 0 ? maxZ : maxY;
                const int other = a == 0 ? maxY : maxZ;
                const int W = h->gauss_w ? h->gauss_w : col_width(Lm);
                dim3 g((unsigned)((int64_t)other * ((maxX + W - 1) / W)), nb);
                const size_t lds = (size_t)Lm * W * 4;
                auto kern = W == 32 ? kGaussColR32[r] : (W == 16 ? kGaussColR16[r] : kGaussColR8[r]);
                lds_optin(kern, lds);
                hipLaunchKernelGGL(kern, g, dim3(256), lds, h->stream, w.desc, w.stat, gp, hp, (const double*)dtaps,
                                   in, (const float*)w.dt, (const uint32_t*)w.smin, (const uint32_t*)w.smax, out);
            }
        } else if (a == 2) {
            dim3 g((unsigned)(((int64_t)maxZ * maxY + 3) / 4), nb);
            const size_t lds = 2 * 128 * 4 + 4 * (size_t)maxX * 4;
            if (lds > 65536)
                (void)hipFuncSetAttribute((const void*)k_gauss_row, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            k_gauss_row<<<g, 256, lds, h->stream>>>(w.desc, w.stat, gp, hp, dtaps, in, w.dt, w.smin, w.smax, out);
        } else {
            const int Lm = a == 0 ? maxZ : maxY;
            const int other = a == 0 ? maxY : maxZ;
            const int W = col_width(Lm);
            dim3 g((unsigned)((int64_t)other * ((maxX + W - 1) / W)), nb);
            const size_t lds = 2 * 128 * 4 + (size_t)Lm * W * 4;
            if (W == 32) lds_optin(k_gauss_col<32>, lds);
            else if (W == 16) lds_optin(k_gauss_col<16>, lds);
            else lds_optin(k_gauss_col<8>, lds);
            if (W == 32)
                k_gauss_col<32><<<g, 256, lds, h->stream>>>(w.desc, w.stat, gp, hp, dtaps, in, w.dt, w.smin, w.smax,
                                                            out);
            else if (W == 16)
                k_gauss_col<16><<<g, 256, lds, h->stream>>>(w.desc, w.stat, gp, hp, dtaps, in, w.dt, w.smin, w.smax,
                                                            out);
            else
                k_gauss_col<8><<<g, 256, lds, h->stream>>>(w.desc, w.stat, gp, hp, dtaps, in, w.dt, w.smin, w.smax,
                                                           out);
        }
        LAUNCHCHK();
        cur = out;
    }
    return CTWS_OK;
}

int cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- flood rounds until no tile is active -----------------------------------------------
// tile extents of k_flood_packed (PTile) and k_flood (FloodTile)
// frontier chunk bricks instantiated in k_flood.hip (CTWS_FRONTIER_SHAPES below): index or -1
// the built bricks: the defaults (2-D 1x64x1, 3-D 1x8x8, masked 3-D 1x32x2) and one alternative
// per dimension for the schedule-independence tests (tests/test_frontier_variants.py); the other
// shapes measured within +-0.1 ms of the defaults (r03) and were dropped from the build
int frontier_chunk_kind(int nd, int cw, int cy, int cz) {
    static const int shapes[5][4] = {{2, 1, 64, 1}, {2, 4, 16, 1}, {3, 1, 8, 8}, {3, 8, 8, 1}, {3, 1, 32, 2}};
    for (int k = 0; k < 5; ++k)
        if (shapes[k][0] == nd && shapes[k][1] == cw && shapes[k][2] == cy && shapes[k][3] == cz) return k;
    return -1;
}
bool frontier_chunk_ok(int nd, int cw, int cy, int cz) { return frontier_chunk_kind(nd, cw, cy, cz) >= 0; }

void flood_tile_dims(int nd, bool packed, int* tz, int* ty, int* tx) {
    *tz = nd == 3 ? (packed ? 16 : 4) : (packed ? 4 : 1);
    *ty = nd == 3 ? (packed ? 16 : 8) : 32;
    *tx = packed ? (nd == 3 ? 16 : 32) : 64;
}

// preset: act0 already holds the tiles to solve in the first round (regrow); otherwise all.
int run_flood(ctws_handle* h, int nd, bool packed, int nb, int max_tiles, int64_t ntiles, const float* hm,
              bool preset, int* rounds_out, float* kernel_ms) {
    Workspace& w = h->ws;
    if (!h->fev[0]) {
        hipEventCreate(&h->fev[0]);
        hipEventCreate(&h->fev[1]);
    }
    float kms = 0.f;
    uint32_t tiles_solved = 0, local_iters = 0;
    if (!preset) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)w.act0, 8u, (size_t)ntiles, h->stream));  // full solve
    HIPCHK(hipMemsetAsync(w.act1, 0, sizeof(uint32_t) * (size_t)ntiles, h->stream));
    HIPCHK(hipMemsetAsync(w.lines0, 0, sizeof(uint32_t) * kLineWords * (size_t)ntiles, h->stream));
    HIPCHK(hipMemsetAsync(w.lines1, 0, sizeof(uint32_t) * kLineWords * (size_t)ntiles, h->stream));
    uint32_t* cur = w.act0;
    uint32_t* nxt = w.act1;
    uint32_t* lcur = w.lines0;  // consumed (and cleared) by the packed kernel
    uint32_t* lnxt = w.lines1;
    dim3 g((unsigned)max_tiles, nb);
    int round = 0;
    for (; round < 1000000; ++round) {
        HIPCHK(hipMemsetAsync(w.counter, 0, kCounterBytes, h->stream));
        hipEventRecord(h->fev[0], h->stream);
        if (packed && nd == 3)
            k_flood_packed<3><<<g, 256, 0, h->stream>>>(w.desc, w.stat, hm, w.key, w.cls, cur, nxt, lcur, lnxt,
                                                        w.counter);
        else if (packed)
            k_flood_packed<2><<<g, 128, 0, h->stream>>>(w.desc, w.stat, hm, w.key, w.cls, cur, nxt, lcur, lnxt,
                                                        w.counter);
        else if (nd == 3)
            k_flood<3><<<g, 256, 0, h->stream>>>(w.desc, w.stat, hm, w.key, w.lab, cur, nxt, w.counter);
        else
            k_flood<2><<<g, 256, 0, h->stream>>>(w.desc, w.stat, hm, w.key, w.lab, cur, nxt, w.counter);
        LAUNCHCHK();
        hipEventRecord(h->fev[1], h->stream);
        HIPCHK(hipMemcpyAsync(h->h_counter, w.counter, kCounterBytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (int k = 1; k < 4; ++k) {
            uint32_t t = 0;
            for (int sl = 0; sl < kStatSlots; ++sl) t += h->h_counter[4 + sl * 4 + k];
            h->h_counter[k] = t;
        }
        float ms = 0.f;
        hipEventElapsedTime(&ms, h->fev[0], h->fev[1]);
        kms += ms;
        tiles_solved += h->h_counter[1];
        local_iters += h->h_counter[2];
        if (h->trace)
            fprintf(stderr, "[ctws] flood%s round %d: %.3f ms, tiles %u, sweeps %u, lines %u, next %u\n",
                    preset ? " (regrow)" : "", round, ms, h->h_counter[1], h->h_counter[2], h->h_counter[3],
                    h->h_counter[0]);
        h->flood_lines += h->h_counter[3];
        if (*h->h_counter == 0) break;
        HIPCHK(hipMemsetAsync(cur, 0, sizeof(uint32_t) * (size_t)ntiles, h->stream));
        std::swap(cur, nxt);
        std::swap(lcur, lnxt);
    }
    if (rounds_out) *rounds_out = round + 1;
    if (kernel_ms) *kernel_ms = kms;
    h->flood_tiles += tiles_solved;
    h->flood_iters += local_iters;
    return CTWS_OK;
}

// Frontier relaxation (k_frontier) from the open / changed bitmaps in w.fopen / w.front0 (written
// by k_descent_init for the first flood, by k_regrow_init for the size-filter regrow) until no
// key changes.  Batches of kFrontierBatch launches run between host checks of their flags; if
// it has not converged after frontier_max_iters iterations (very long equal-height paths) the
// tile flood finishes from the current keys.
int run_frontier(ctws_handle* h, const Plan& pl, int nb, int64_t TF, int max_tiles, int64_t TT, bool packed,
                 uint32_t* fst, int* iters_out, int* rounds_out, float* kms_out, bool regrow = false) {
    Workspace& w = h->ws;
    const int64_t nch = (TF >> kChunkShift) + 1;
    uint64_t* fb[2] = {w.front0, w.front1};  // changed bitmaps: iteration it reads fb[it & 1]
    uint32_t* gen[2] = {w.fchunk0, w.fchunk1};  // iteration it writes gen[it & 1], reads gen[(it + 1) & 1]
    uint32_t* wl[2] = {w.wl0, w.wl1};
    HIPCHK(hipMemsetAsync(w.fchunk0, 0, sizeof(uint32_t) * (size_t)nch, h->stream));
    HIPCHK(hipMemsetAsync(w.fchunk1, 0, sizeof(uint32_t) * (size_t)nch, h->stream));
    HIPCHK(hipMemsetAsync(w.qgen, 0, sizeof(uint32_t) * (size_t)nch, h->stream));
    HIPCHK(hipMemsetAsync(w.wlcnt, 0, sizeof(uint32_t) * (size_t)(h->frontier_max_iters + 2), h->stream));
    // iteration 0: every chunk with an open voxel
    const dim3 lg((unsigned)std::min<int64_t>((TF / nb + 64 * 64 * kFrontierWavesHost - 1) / (64 * 64 * kFrontierWavesHost) + 1,
                                              1024), nb);
    const int* fc = h->fc_cur;
    const int fkind = frontier_chunk_kind(pl.nd_ws, fc[0], fc[1], fc[2]);
#define CTWS_FRONTIER_SHAPES(X) X(0, 2, 1, 64, 1) X(1, 2, 4, 16, 1) X(2, 3, 1, 8, 8) X(3, 3, 8, 8, 1) X(4, 3, 1, 32, 2)
#define CTWS_LIST0(K, ND, CW, CY, CZ) \
    case K: k_frontier_list0<CW, CY, CZ><<<lg, 256, 0, h->stream>>>(w.desc, w.stat, w.fopen, wl[0], w.wlcnt); break;
    switch (fkind) {
        CTWS_FRONTIER_SHAPES(CTWS_LIST0)
        default: h->err = "bad frontier chunk"; return CTWS_EINVAL;
    }
#undef CTWS_LIST0
    LAUNCHCHK();
    // one wave per list entry; the largest list is every chunk of the batch
    const unsigned fg = (unsigned)std::min<int64_t>((nch + kFrontierWavesHost - 1) / kFrontierWavesHost, h->frontier_grid);
    bool converged = false;
    int fiters = 0;
    while (fiters < h->frontier_max_iters && !converged) {
        const int it0 = fiters;
        const int nl = std::min(kFrontierBatch, h->frontier_max_iters - it0);
        std::vector<hipEvent_t> tev;
        if (h->trace) {
            tev.resize(nl + 1);
            for (auto& e : tev) hipEventCreate(&e);
            hipEventRecord(tev[0], h->stream);
        }
        for (int k = 0; k < nl; ++k) {
            const int it = it0 + k;
#define CTWS_FRONTIER(K, ND, CW, CY, CZ)                                                                            \
    case K:                                                                                                         \
        k_frontier<ND, CW, CY, CZ><<<fg, 256, 0, h->stream>>>(                                                      \
            w.desc, w.stat, w.hm, w.key, w.fopen, fb[it & 1], fb[(it + 1) & 1], gen[(it + 1) & 1], gen[it & 1], it, \
            wl[it & 1], w.wlcnt + it, wl[(it + 1) & 1], w.wlcnt + it + 1, w.qgen, fst ? fst + nb : nullptr,         \
            h->frontier_reps, h->frontier_dir);                                                                     \
        break;
            switch (fkind) {
                CTWS_FRONTIER_SHAPES(CTWS_FRONTIER)
            }
#undef CTWS_FRONTIER
            if (h->trace) hipEventRecord(tev[k + 1], h->stream);
        }
        LAUNCHCHK();
        HIPCHK(hipMemcpyAsync(h->h_counter, w.wlcnt + it0, sizeof(uint32_t) * (nl + 1), hipMemcpyDeviceToHost,
                              h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->trace) {
            for (int k = 0; k < nl; ++k) {
                float ms = 0.f;
                hipEventElapsedTime(&ms, tev[k], tev[k + 1]);
                std::fprintf(stderr, "[ctws] frontier it %d: %u chunks, %.3f ms\n", it0 + k, h->h_counter[k], ms);
                if (!h->h_counter[k + 1]) break;
            }
            for (auto& e : tev) hipEventDestroy(e);
        }
        std::memmove(h->h_counter, h->h_counter + 1, sizeof(uint32_t) * nl);
        for (int k = 0; k < nl; ++k) {
            ++fiters;
            if (!h->h_counter[k]) {  // nothing queued for the next iteration
                converged = true;
                break;
            }
        }
    }
#undef CTWS_FRONTIER_SHAPES
    *iters_out += fiters;
    if (!converged) {
        int TZ, TY, TX;
        flood_tile_dims(pl.nd_ws, packed, &TZ, &TY, &TX);
        HIPCHK(hipMemsetAsync(w.act0, 0, sizeof(uint32_t) * (size_t)TT, h->stream));
        k_frontier_tiles<<<dim3((unsigned)std::min<int64_t>((TF / nb + 255) / 256 + 1, 4096), nb), 256, 0,
                           h->stream>>>(w.desc, w.stat, w.fopen, w.act0, TZ, TY, TX);
        // a sparse regrow (k_sf_sparse) left the survivors' seed flags as the first flood had
        // them: the tile flood needs every survivor fixed
        if (regrow) k_fixed_from_open<<<dim3(2048, nb), 256, 0, h->stream>>>(w.desc, w.stat, w.fopen, w.cls);
        LAUNCHCHK();
        int rounds = 0;
        float kms = 0.f;
        int r = run_flood(h, pl.nd_ws, packed, nb, max_tiles, TT, w.hm, true, &rounds, &kms);
        if (r != CTWS_OK) return r;
        *rounds_out += rounds;
        *kms_out += kms;
    }
    return CTWS_OK;
}



void add_timing(ctws_handle* h, const char* name, float v);

int64_t words_of(int64_t n) { return n / 64 + 1; }
int64_t chunks_of(int64_t n) { return (words_of(n) + 255) / 256; }

// timings of one ctws_ws_blocks call: summed over its batches (counts too)
void add_timing(ctws_handle* h, const char* name, float v) {
    for (auto& t : h->timings)
        if (std::strcmp(t.first, name) == 0) {
            t.second += v;
            return;
        }
    h->timings.push_back({name, v});
}

// an entry that names something of the last batch (prep_kernel): replaced, not summed
void set_timing(ctws_handle* h, const char* name, float v) {
    for (auto& t : h->timings)
        if (std::strcmp(t.first, name) == 0) {
            t.second = v;
            return;
        }
    h->timings.push_back({name, v});
}

// ---- WatershedFromSeeds seeds (k_seeded.hip) ----------------------------------------------
// The blocks' distinct seed values (hash), sorted per block (segmented radix sort), a label
// per value = 1 + its rank; blocks without any seed get the strict minima of the hmap
// (k_auto_minima + the bitmap rank, labels written by k_fs_auto_label once `packed` is known).
template <class V>
int fs_seeds(ctws_handle* h, const std::vector<BlockDesc>& desc, int nb, int64_t TH, int64_t TW, int64_t TS,
             int64_t maxH, int64_t maxRows, dim3 vg, dim3 wg, V /* value type: uint32_t or uint64_t */) {
    Workspace& w = h->ws;
    int r;
    const size_t nh = (size_t)std::max<int64_t>(TH, 1);
    if ((r = grow(h, h->fs_vals, sizeof(V) * nh)) != CTWS_OK) return r;
    if ((r = grow(h, h->fs_sorted, sizeof(V) * nh)) != CTWS_OK) return r;
    if ((r = grow(h, h->fs_off, sizeof(int) * 2 * (size_t)nb)) != CTWS_OK) return r;
    V* vals = (V*)h->fs_vals.p;
    V* sorted = (V*)h->fs_sorted.p;
    int* off = (int*)h->fs_off.p;
    HIPCHK(hipMemsetAsync(w.hkey, 0xFF, sizeof(uint64_t) * nh, h->stream));
    k_fs_insert<V><<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.hkey);
    const dim3 hg((unsigned)std::min<int64_t>((maxH + 255) / 256, 4096), nb);
    k_fs_collect<V><<<hg, 256, 0, h->stream>>>(w.desc, w.stat, w.hkey, vals);
    k_fs_offsets<<<(nb + 255) / 256, 256, 0, h->stream>>>(w.desc, w.stat, nb, off, off + nb);
    LAUNCHCHK();
    size_t tb = 0;
    HIPCHK(fs_segmented_sort(nullptr, tb, vals, sorted, (int)nh, nb, off, off + nb, h->stream));
    if ((r = grow(h, h->fs_tmp, tb)) != CTWS_OK) return r;
    HIPCHK(fs_segmented_sort(h->fs_tmp.p, tb, vals, sorted, (int)nh, nb, off, off + nb, h->stream));
    k_fs_rank<V><<<hg, 256, 0, h->stream>>>(w.desc, w.stat, w.hkey, sorted, w.hpos);
    LAUNCHCHK();
    std::vector<BlockStat> st(nb);
    HIPCHK(hipMemcpyAsync(st.data(), w.stat, sizeof(BlockStat) * nb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    std::vector<uint32_t> surv((size_t)std::max<int64_t>(TS, 1), 1u);
    bool any = false;
    for (int i = 0; i < nb; ++i)
        if (st[i].n_seeds == 0) {
            surv[desc[i].sbase] = 0u;
            any = true;
        }
    HIPCHK(hipMemcpyAsync(w.surv, surv.data(), sizeof(uint32_t) * surv.size(), hipMemcpyHostToDevice, h->stream));
    if (any) {
        // watershedsNew with an all-zero seed image seeds from the strict minima of the hmap
        HIPCHK(hipMemsetAsync(w.W, 0, sizeof(uint64_t) * (size_t)TW, h->stream));
        const dim3 ag((unsigned)std::min<int64_t>(maxRows, 65535), nb);
        k_auto_minima<<<ag, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.surv, w.W);
        k_bitmap_csum<<<wg, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.W, w.csum);
        k_chunk_scan<<<nb, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.csum, 2);
        k_word_prefix<<<wg, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.W, w.csum, w.Wp);
        LAUNCHCHK();
    }
    // (surv stays in w.surv: k_fs_auto_label reads it; the size filter re-initialises it)
    return CTWS_OK;
}

// ---- one batch, all pointers on the device ------------------------------------------------
int run_batch(ctws_handle* h, const ctws_cfg* cfg, const Plan& pl, ctws_block* blocks, const BlockIO* io, int nb) {
    Workspace& w = h->ws;
    std::vector<BlockDesc> desc(nb);
    int64_t T = 0, TI = 0, TW = 0, TC = 0, TS = 0, TT = 0, TH = 0, TF = 0;
    int64_t maxH = 0, maxRows = 0, maxIRows = 0;
    int maxZ = 0, maxY = 0, maxX = 0, max_tiles = 0;
    int64_t maxN = 0, maxNI = 0;
    int maxIZ = 0, maxIY = 0, maxIX = 0;
    bool real_edt = pl.real_pitch;  // the batch's distances take vigra's real-valued path
    bool real_double = pl.real_pitch;  // ... with a double temporary (else float)
    const uint64_t bvol = (uint64_t)(cfg->block_shape[0] * cfg->block_shape[1] * cfg->block_shape[2]);
    {
        bool any_mask = false;
        for (int i = 0; i < nb; ++i) any_mask |= io[i].mask != nullptr;
        const int* fc = pl.nd_ws == 2 ? h->fchunk2 : (any_mask && !h->fchunk3_env ? h->fchunk3_masked : h->fchunk3);
        std::memcpy(h->fc_cur, fc, sizeof(h->fc_cur));
    }
    for (int i = 0; i < nb; ++i) {
        const ctws_block& b = blocks[i];
        BlockDesc& d = desc[i];
        std::memset(&d, 0, sizeof(d));
        d.Z = (int)b.outer_shape[0];
        d.Y = (int)b.outer_shape[1];
        d.X = (int)b.outer_shape[2];
        d.nd_ws = pl.nd_ws;
        d.N = (int64_t)d.Z * d.Y * d.X;
        d.base = T;
        d.iz0 = (int)b.inner_begin[0];
        d.iy0 = (int)b.inner_begin[1];
        d.ix0 = (int)b.inner_begin[2];
        d.IZ = (int)b.inner_shape[0];
        d.IY = (int)b.inner_shape[1];
        d.IX = (int)b.inner_shape[2];
        d.NI = (int64_t)d.IZ * d.IY * d.IX;
        d.crop = b.crop_relabel ? 1 : 0;
        d.ibase = T;  // inner arrays reuse the outer-sized parent array (NI <= N)
        d.wbase = TW;
        d.cbase = TC;
        d.sbase = TS;
        d.input = io[i].in;
        d.mask = io[i].mask;
        d.init = io[i].init;
        d.out = io[i].out;
        d.out32 = io[i].out32;
        d.n_channels = b.n_channels;
        d.dtype = b.input_dtype;
        if (b.n_channels > 0) {
            int cb = cfg->channel_begin, ce = cfg->channel_end < 0 ? b.n_channels : cfg->channel_end;
            if (cb < 0) cb += b.n_channels;
            if (ce > b.n_channels) ce = b.n_channels;
            if (cb > ce) cb = ce;
            d.c0 = cb;
            d.C = ce - cb;
            if (d.C <= 0) {
                h->err = "empty channel range";
                return CTWS_EINVAL;
            }
        } else {
            d.c0 = 0;
            d.C = 1;
        }
        d.id_offset = (uint64_t)b.block_id * bvol;
        d.pass2 = (uint32_t)pl.pass2;
        d.p2hint = -1;
        if (pl.pass2 || pl.from_seeds) {
            if (!d.init) {
                h->err = "pass 2 needs initial_seeds (ds_out[input_bb]) for every block";
                return CTWS_EINVAL;
            }
            int64_t cap = 4096;
            while (cap < d.N / 4) cap <<= 1;
            d.hbase = TH;
            d.hcap = cap;
            TH += cap;
        }
        d.maxd = (uint32_t)std::min<int64_t>((int64_t)pl.pitch[0] * pl.pitch[0] * d.Z * d.Z +
                                                 (int64_t)pl.pitch[1] * pl.pitch[1] * d.Y * d.Y +
                                                 (int64_t)pl.pitch[2] * pl.pitch[2] * d.X * d.X, 0xFFFFFFFFll);
        d.fbase = TF;
        // frontier bitmaps: rows padded to a multiple of 64, and at least 64 words per frontier
        // chunk brick (k_frontier), so that the per-chunk arrays can be indexed at fbase / 64
        {
            const int* fc = h->fc_cur;
            const int64_t wpr = (d.X + 63) / 64;
            const int64_t nch = ((wpr + fc[0] - 1) / fc[0]) * ((d.Y + fc[1] - 1) / fc[1]) * ((d.Z + fc[2] - 1) / fc[2]);
            TF += std::max((((int64_t)d.Z * d.Y + 63) / 64) * 64 * wpr, nch << kChunkShift);
        }
        T += d.N;
        TI += d.NI;
        TW += words_of(d.N);
        TC += chunks_of(d.N);
        TS += d.Z;
        maxZ = std::max(maxZ, d.Z);
        maxY = std::max(maxY, d.Y);
        maxX = std::max(maxX, d.X);
        maxN = std::max(maxN, d.N);
        maxNI = std::max(maxNI, d.NI);
        maxIZ = std::max(maxIZ, d.IZ);
        maxIY = std::max(maxIY, d.IY);
        maxIX = std::max(maxIX, d.IX);
        maxH = std::max(maxH, d.hcap);
        maxRows = std::max(maxRows, (int64_t)d.Z * d.Y);
        maxIRows = std::max(maxIRows, (int64_t)d.IZ * d.IY);
        // validation against what the kernels assume (run_blocks already failed such blocks
        // individually, block_refusal)
        if (d.X > kMaxRowX || d.Y > kMaxColLen || d.Z > kMaxColLen || d.N >= (1ll << 31)) {
            h->err = "outer block too large for the kernels (X <= 10176, Y, Z <= 5088, N < 2^31)";
            return CTWS_EUNSUPPORTED;
        }
        if (d.iz0 < 0 || d.iy0 < 0 || d.ix0 < 0 || d.iz0 + d.IZ > d.Z || d.iy0 + d.IY > d.Y || d.ix0 + d.IX > d.X ||
            d.IZ <= 0 || d.IY <= 0 || d.IX <= 0) {
            h->err = "inner block outside the outer block";
            return CTWS_EINVAL;
        }
        if (!d.input || (!d.out && !d.out32)) {
            h->err = "null input/output";
            return CTWS_EINVAL;
        }
        // vigra's convolveLine needs line length > kernel radius
        auto chk_len = [&](const double* sg, bool en) -> bool {
            if (!en) return true;
            const int lens[3] = {d.Z, d.Y, d.X};
            for (int a = (pl.nd_ws == 3 ? 0 : 1); a < 3; ++a) {
                if (sg[a] <= 0) continue;
                int r = (int)(3.0 * sg[a] + 0.5);
                if (r == 0) r = 1;
                if (lens[a] < r + 1) return false;
            }
            return true;
        };
        if (!chk_len(pl.sig_seeds, pl.seeds_smooth) || !chk_len(pl.sig_weights, pl.weights_smooth)) {
            h->err = "convolveLine(): kernel longer than line";
            return CTWS_EINVAL;
        }
        double dmax;
        if (pl.dt_2d) dmax = (double)d.Y * d.Y + (double)d.X * d.X;
        else
            dmax = std::pow(pl.pitchd[0] * d.Z, 2) + std::pow(pl.pitchd[1] * d.Y, 2) + std::pow(pl.pitchd[2] * d.X, 2);
        // dmax >= 2^24: float32 squared distances are no longer exact integers; vigra's float
        // arithmetic is then reproduced by the real-valued path (k_edt_real_*)
        if (dmax >= 16777216.0 && !pl.from_seeds) real_edt = true;
        if (dmax > 3.4028234663852886e38 && !pl.from_seeds) real_double = true;  // > FLT_MAX: double, as vigra
    }
    // flood tile grids: the largest (wide kernel) bounds the per-tile arrays
    auto set_tiles = [&](bool packed) {
        int TZ, TY, TX;
        flood_tile_dims(pl.nd_ws, packed, &TZ, &TY, &TX);
        TT = 0;
        max_tiles = 0;
        for (auto& d : desc) {
            d.tz = (d.Z + TZ - 1) / TZ;
            d.ty = (d.Y + TY - 1) / TY;
            d.tx = (d.X + TX - 1) / TX;
            d.tbase = (int)TT;
            TT += (int64_t)d.tz * d.ty * d.tx;
            max_tiles = std::max(max_tiles, d.tz * d.ty * d.tx);
        }
    };
    // crop CC: each cropped block's tiles get 2 x columns of (root, label) entries (k_tile_cc)
    int64_t TXF = 0;
    {
        const int ctz = pl.nd_ws == 3 ? CcTile<3>::TZ : CcTile<2>::TZ;
        const int cty = pl.nd_ws == 3 ? CcTile<3>::TY : CcTile<2>::TY;
        const int ctx = pl.nd_ws == 3 ? CcTile<3>::TX : CcTile<2>::TX;
        for (auto& d : desc) {
            d.xcbase = TXF;
            if (d.crop) TXF += (int64_t)cdiv(d.IZ, ctz) * cdiv(d.IY, cty) * cdiv(d.IX, ctx) * 2 * ctz * cty;
        }
    }
    // plateau CC: one flag per tile (k_localmax sets it for the tiles with a plateau voxel)
    int64_t TPT = 0;
    {
        const int ptz = pl.nd_ws == 3 ? CcTileM<3, CC_PLATEAU>::TZ : CcTileM<2, CC_PLATEAU>::TZ;
        const int pty = pl.nd_ws == 3 ? CcTileM<3, CC_PLATEAU>::TY : CcTileM<2, CC_PLATEAU>::TY;
        const int ptx = pl.nd_ws == 3 ? CcTileM<3, CC_PLATEAU>::TX : CcTileM<2, CC_PLATEAU>::TX;
        for (auto& d : desc) {
            d.ptbase = TPT;
            TPT += (int64_t)cdiv(d.Z, ptz) * cdiv(d.Y, pty) * cdiv(d.X, ptx);
        }
    }
    h->last_bare.assign(nb, 1);  // (a run stopped early by a test hook writes no labels)
    h->cur_max[0] = maxZ;
    h->cur_max[1] = maxY;
    h->cur_max[2] = maxX;
    set_tiles(true);
    const int64_t TT_packed = TT;
    set_tiles(false);
    const int64_t TT_wide = TT;
    set_tiles(true);
    int r;
    if ((r = ensure_workspace(h, T, TW, TC, TS, std::max(TT_packed, TT_wide), nb, TH, TF)) != CTWS_OK) return r;
    if (TXF && (r = grow(h, h->xface, sizeof(uint64_t) * (size_t)TXF)) != CTWS_OK) return r;
    if ((r = grow(h, h->ptile, sizeof(uint32_t) * (size_t)std::max<int64_t>(TPT, 1))) != CTWS_OK) return r;
    if (pl.pass2 && pl.nd_ws == 2 && (int)h->p2_hints.size() == nb) {
        std::vector<uint32_t> flat;
        for (int i = 0; i < nb; ++i) {
            if ((int)h->p2_hints[i].size() != desc[i].Z) continue;
            desc[i].p2hint = (int64_t)flat.size();
            flat.insert(flat.end(), h->p2_hints[i].begin(), h->p2_hints[i].end());
        }
        if (!flat.empty()) {
            if ((r = grow(h, h->p2_hint_dev, sizeof(uint32_t) * flat.size())) != CTWS_OK) return r;
            HIPCHK(hipMemcpy(h->p2_hint_dev.p, flat.data(), sizeof(uint32_t) * flat.size(), hipMemcpyHostToDevice));
        }
    }
    HIPCHK(hipMemcpyAsync(w.desc, desc.data(), sizeof(BlockDesc) * nb, hipMemcpyHostToDevice, h->stream));
    h->last_desc = desc;
    std::vector<BlockStat> st(nb);
    for (auto& s : st) {
        std::memset(&s, 0, sizeof(s));
        s.in_min = 0xFFFFFFFFu;
        s.dt_min = 0xFFFFFFFFu;
    }
    HIPCHK(hipMemcpyAsync(w.stat, st.data(), sizeof(BlockStat) * nb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)w.smin, 0xFFFFFFFFu, (size_t)TS, h->stream));
    HIPCHK(hipMemsetAsync(w.smax, 0, sizeof(uint32_t) * TS, h->stream));
    HIPCHK(hipMemsetAsync(w.slmax, 0, sizeof(uint32_t) * TS, h->stream));
    HIPCHK(hipMemsetAsync(w.surv, 0, sizeof(uint32_t) * TS, h->stream));

    const dim3 vg((unsigned)std::min<int64_t>((maxN + 255) / 256, 4096), nb);
    const dim3 ig((unsigned)std::min<int64_t>((maxNI + 255) / 256, 4096), nb);
    // 4 voxels per thread (16-byte groups)
    const dim3 vg4((unsigned)std::min<int64_t>((maxN / 4 + 256) / 256, 4096), nb);
    const dim3 wg((unsigned)((words_of(maxN) + 255) / 256), nb);
    // row-tile kernels: kRows rows (z, y) per workgroup iteration
    const dim3 rg((unsigned)std::min<int64_t>((maxRows + kRows - 1) / kRows, 16384), nb);
    const dim3 rig((unsigned)std::min<int64_t>((maxIRows + kRows - 1) / kRows, 16384), nb);
    // word-tile kernels: one wave per 64-voxel row word, kWordWaves waves per workgroup
    // (h->words_per_wave words per wave: a workgroup per handful of words would make the
    // dispatch of ~10^6 workgroups the bottleneck)
    const int64_t wpw = (int64_t)kWordWaves * h->words_per_wave;
    // (x extents rounded to a multiple of 8: xcd_swizzle's id % 8 then labels one XCD per grid row)
    auto r8 = [](int64_t v) { return (unsigned)std::min<int64_t>(v > 8 ? (v + 7) / 8 * 8 : v, 65528); };
    // one workgroup per tile, rounded up to a multiple of 8 for xcd_swizzle (no cap: every tile
    // needs its workgroup; the extra ones return at once)
    auto tiles8 = [](int64_t v) { return (unsigned)(v > 8 ? (v + 7) / 8 * 8 : v); };
    const dim3 wtg(r8((maxRows * ((maxX + 63) / 64) + wpw - 1) / wpw), nb);
    const dim3 wtig(r8((maxIRows * ((maxIX + 63) / 64) + wpw - 1) / wpw), nb);
    size_t ev = 0;
    std::vector<const char*> names;
    auto mark = [&](const char* name) {
        record(h, ev++);
        names.push_back(name);
    };
    mark("start");

    // ---- normalize + threshold + EDT ------------------------------------------------------
    // typed batches on the integer EDT hand the rows' foreground bits to the y pass (one EdtRec
    // per word, in w.key: free until the seeds are labelled) instead of g2 per voxel in w.A
    bool edt_bits = false;
    EdtRec* const edt_rec = (EdtRec*)w.key;
    // the x-pass kernel of this batch, for ctws_last_timings (include/ctws.h): 0 the generic LDS
    // kernel, KMAX (+ 100 with BITS) k_prep_edt_x_co, 200 + KMAX k_prep_edt_x_reg, -1 the fill
    int prep_kernel = 0;
    if (pl.sf_fill) {
        prep_kernel = -1;
        // the height map as it is stored: no min / max, normalize or EDT pass
        k_sf_hmap<<<vg, 256, 0, h->stream>>>(w.desc, w.hm);
        k_fs_active<<<(nb + 255) / 256, 256, 0, h->stream>>>(w.desc, w.stat, nb);
        LAUNCHCHK();
    } else {
        // one raw dtype and 3-D datasets in the batch: the typed kernels (global loads in flight)
        int dt = desc[0].dtype;
        bool typed = !h->prep_lds && maxX <= 1024;
        bool all_exact = true;
        for (auto& d : desc) {
            typed &= d.dtype == dt && d.n_channels == 0;
            all_exact &= d.X == maxX && (d.X == 256 || d.X == 512 || d.X == 1024) && d.n_channels == 0 && d.dtype == 3;
        }
        edt_bits = h->edt_bits && typed && !real_edt && !pl.from_seeds && 2 * TF <= T;
        dim3 g((unsigned)std::min<int64_t>((maxN + 65535) / 65536, 256), nb);
        if (typed) {
            dim3 gm((unsigned)std::min<int64_t>((maxN + 8 * 256 - 1) / (8 * 256), 1024), nb);
            if (dt == CTWS_U8) k_input_minmax_t<uint8_t><<<gm, 256, 0, h->stream>>>(w.desc, w.stat);
            else if (dt == CTWS_U16) k_input_minmax_t<uint16_t><<<gm, 256, 0, h->stream>>>(w.desc, w.stat);
            else if (dt == CTWS_F32) k_input_minmax_t<float><<<gm, 256, 0, h->stream>>>(w.desc, w.stat);
            else k_input_minmax_t<double><<<gm, 256, 0, h->stream>>>(w.desc, w.stat);
        } else {
            k_input_minmax<<<g, 256, 0, h->stream>>>(w.desc, w.stat);
        }
        LAUNCHCHK();
        // WatershedFromSeeds: _read_data without invert; the normalized input is the hmap
        PrepParams pp{(float)cfg->threshold, pl.from_seeds ? 0 : cfg->invert_inputs, cfg->agglomerate_channels,
                      pl.pitch[2] * pl.pitch[2]};
        float* fin_out = pl.from_seeds ? w.hm : w.fin;
        dim3 gx((unsigned)(((int64_t)maxZ * maxY + 3) / 4), nb);
        // rows up to 1024 voxels: one wave per row in registers.  f32 rows of exactly 64 K voxels
        // move as float4 with lanes owning consecutive voxels (k_prep_edt_x_reg); other rows use
        // the lane-interleaved coalesced layout (k_prep_edt_x_co)
        auto launch_co = [&](auto kmax_c, auto bits_c) {
            constexpr int KM = decltype(kmax_c)::value;
            constexpr bool BITS = decltype(bits_c)::value;
            prep_kernel = KM + (BITS ? 100 : 0);
            auto go = [&](auto kern) { kern<<<gx, 256, 0, h->stream>>>(w.desc, w.stat, pp, fin_out, (uint32_t*)w.A, edt_rec); };
            if (dt == CTWS_U8) go(k_prep_edt_x_co<KM, uint8_t, BITS>);
            else if (dt == CTWS_U16) go(k_prep_edt_x_co<KM, uint16_t, BITS>);
            else if (dt == CTWS_F32) go(k_prep_edt_x_co<KM, float, BITS>);
            else go(k_prep_edt_x_co<KM, double, BITS>);
        };
        if (edt_bits && maxX <= 256)
            launch_co(std::integral_constant<int, 4>(), std::true_type());
        else if (edt_bits && maxX <= 512)
            launch_co(std::integral_constant<int, 8>(), std::true_type());
        else if (edt_bits)
            launch_co(std::integral_constant<int, 16>(), std::true_type());
        else if (typed && all_exact && maxX == 256) {
            prep_kernel = 200 + 4;
            k_prep_edt_x_reg<4><<<gx, 256, 0, h->stream>>>(w.desc, w.stat, pp, fin_out, (uint32_t*)w.A);
        } else if (typed && all_exact && maxX == 512) {
            prep_kernel = 200 + 8;
            k_prep_edt_x_reg<8><<<gx, 256, 0, h->stream>>>(w.desc, w.stat, pp, fin_out, (uint32_t*)w.A);
        } else if (typed && all_exact && maxX == 1024) {
            prep_kernel = 200 + 16;
            k_prep_edt_x_reg<16><<<gx, 256, 0, h->stream>>>(w.desc, w.stat, pp, fin_out, (uint32_t*)w.A);
        } else if (typed && maxX <= 256)
            launch_co(std::integral_constant<int, 4>(), std::false_type());
        else if (typed && maxX <= 512)
            launch_co(std::integral_constant<int, 8>(), std::false_type());
        else if (typed && maxX <= 1024)
            launch_co(std::integral_constant<int, 16>(), std::false_type());
        else {
            lds_optin(k_prep_edt_x, 4 * (size_t)maxX * 4);
            k_prep_edt_x<<<gx, 256, 4 * (size_t)maxX * 4, h->stream>>>(w.desc, w.stat, pp, fin_out, (uint32_t*)w.A);
        }
        LAUNCHCHK();
        if (pl.from_seeds) k_fs_active<<<(nb + 255) / 256, 256, 0, h->stream>>>(w.desc, w.stat, nb);
        else k_set_active<<<(nb + 255) / 256, 256, 0, h->stream>>>(w.desc, w.stat, nb);
        LAUNCHCHK();
    }
    mark("prep_edt_x");
    set_timing(h, "prep_kernel", (float)prep_kernel);
    bool packed = true;
    // the seed stage's passes over the classes: dense, or a walk over k_localmax's equal bitmap
    const bool seed_dense = !pl.from_seeds && (h->seed_dense || h->seed_tilecc);
    uint32_t max_seeds = 0;  // sizes the LDS histogram of the size filter
    std::vector<BlockStat> s2(nb);
    const dim3 gsb((unsigned)((maxZ + 255) / 256), nb);
    if (pl.from_seeds) {
        // the filling size filter keeps the full uint64 ids (k_seeded.hip, value type V)
        r = pl.sf_fill ? fs_seeds(h, desc, nb, TH, TW, TS, maxH, maxRows, vg, wg, uint64_t())
                       : fs_seeds(h, desc, nb, TH, TW, TS, maxH, maxRows, vg, wg, uint32_t());
        if (r != CTWS_OK) return r;
    } else {
    if (real_edt) {
        // vigra's real-valued path: double temporary (non-integer pitch) or float (dmax >= 2^24)
        EdtRealParams er{{pl.pitchd[0], pl.pitchd[1], pl.pitchd[2]}, pl.dt_2d, real_double ? 1 : 0};
        const int nthr = 64 * 256;
        const int maxL = std::max(maxZ, std::max(maxY, maxX));
        const size_t esz = real_double ? 8 : 4;
        if ((r = grow(h, h->edt_scratch, (size_t)nthr * maxL * (2 * esz + 20))) != CTWS_OK) return r;
        char* scr = (char*)h->edt_scratch.p;
        auto run_real = [&](auto tag) {
            using T = decltype(tag);
            T* tmp = (T*)w.key;  // free until the flood
            k_edt_real_init<T><<<vg, 256, 0, h->stream>>>(w.desc, w.stat, er, (const uint32_t*)w.A, tmp);
            for (int a = pl.dt_2d ? 1 : 0; a < 3; ++a)
                k_edt_real_line<T><<<nthr / 256, 256, 0, h->stream>>>(w.desc, w.stat, nb, er, a, tmp, scr, maxL);
            k_edt_real_final<T><<<vg, 256, 0, h->stream>>>(w.desc, w.stat, er, tmp, w.dt, w.smin, w.smax);
        };
        if (real_double) run_real(double());
        else run_real(float());
        LAUNCHCHK();
        if (!pl.dt_2d && pl.nd_ws == 2) {
            dim3 gs((unsigned)maxZ, nb);
            k_dt_slice_stats<<<gs, 256, 0, h->stream>>>(w.desc, w.stat, w.dt, w.smin, w.smax);
            LAUNCHCHK();
        }
    } else {
        // y pass (final for a 2-D dt), then z pass (3-D dt)
        // (a forced width narrows until the column tile fits the LDS: the default already does)
        auto fit = [](int W, int L) {
            while (W > 8 && (size_t)L * W * 4 > kMaxLds) W /= 2;
            return W;
        };
        const int Wy = fit(h->edt_w ? h->edt_w : edt_col_width(maxY), maxY);
        EdtColParams ep{1, pl.pitch[1] * pl.pitch[1], pl.dt_2d, pl.dt_2d, 0u, pl.pitch[2] * pl.pitch[2]};
        dim3 gy((unsigned)((int64_t)maxZ * ((maxX + Wy - 1) / Wy)), nb);
        const size_t ldsy = (size_t)maxY * Wy * 4;
        // columns that may go to the lower-envelope pass: one entry each at most
        int64_t ncols = 0, ncols_z = 0;
        for (auto& d : desc) {
            ncols += (int64_t)d.Z * d.X;
            ncols_z += (int64_t)d.Y * d.X;
        }
        if (!pl.dt_2d) ncols = std::max(ncols, ncols_z);
        if ((r = grow(h, h->edt_fh, 64 + 8 * (size_t)ncols)) != CTWS_OK) return r;
        uint32_t* fh_cnt = (uint32_t*)h->edt_fh.p;
        unsigned long long* fh_list = (unsigned long long*)((char*)h->edt_fh.p + 64);
        HIPCHK(hipMemsetAsync(fh_cnt, 0, 64, h->stream));
        const unsigned gfh = (unsigned)std::min<int64_t>((ncols + 255) / 256, 1024);
        auto launch_col = [&](int W, dim3 g, size_t lds, EdtColParams p, const uint32_t* gin, uint32_t* gout,
                              uint32_t* cnt) {
            auto go = [&](auto kern) {
                lds_optin(kern, lds);
                kern<<<g, 256, lds, h->stream>>>(w.desc, w.stat, p, gin, gout, w.dt, w.smin, w.smax, fh_list, cnt);
            };
            if (W == 64) go(k_edt_col<64>);
            else if (W == 32) go(k_edt_col<32>);
            else if (W == 16) go(k_edt_col<16>);
            else go(k_edt_col<8>);
            k_edt_col_fh<<<gfh, 256, 0, h->stream>>>(w.desc, w.stat, p, gin, nullptr, gout, w.dt, w.smin, w.smax, fh_list, cnt);
        };
        // the record-fed y pass: 16 columns through a ring of 256 rows (16 KiB of LDS whatever
        // the column length; the other tile shapes measured are in DESIGN.md section 3)
        auto launch_col_bits = [&](EdtColParams p, uint32_t* gout, uint32_t* cnt) {
            constexpr int W = 16, RING = 256;
            dim3 g((unsigned)((int64_t)maxZ * ((maxX + W - 1) / W)), nb);
            k_edt_col_bits<W, RING><<<g, 256, (size_t)RING * W * 4, h->stream>>>(w.desc, w.stat, p, edt_rec, gout, w.dt,
                                                                                 w.smin, w.smax, fh_list, cnt);
            k_edt_col_fh<<<gfh, 256, 0, h->stream>>>(w.desc, w.stat, p, nullptr, edt_rec, gout, w.dt, w.smin, w.smax, fh_list, cnt);
        };
        if (edt_bits) launch_col_bits(ep, (uint32_t*)w.Bf, fh_cnt);
        else launch_col(Wy, gy, ldsy, ep, (uint32_t*)w.A, (uint32_t*)w.Bf, fh_cnt);
        LAUNCHCHK();
        if (!pl.dt_2d) {
            const int Wz = fit(h->edt_wz ? h->edt_wz : h->edt_w ? h->edt_w : edt_col_width(maxZ), maxZ);
            dim3 gz((unsigned)((int64_t)maxY * ((maxX + Wz - 1) / Wz)), nb);
            const size_t ldsz = (size_t)maxZ * Wz * 4;
            EdtColParams ez{2, pl.pitch[0] * pl.pitch[0], 1, 0, 0u};
            launch_col(Wz, gz, ldsz, ez, (uint32_t*)w.Bf, nullptr, fh_cnt + 1);
            LAUNCHCHK();
            if (pl.nd_ws == 2) {
                dim3 gs((unsigned)maxZ, nb);
                k_dt_slice_stats<<<gs, 256, 0, h->stream>>>(w.desc, w.stat, w.dt, w.smin, w.smax);
                LAUNCHCHK();
            }
        }
    }
    if (h->trace && !real_edt) {
        uint32_t c[2];
        HIPCHK(hipMemcpy(c, h->edt_fh.p, sizeof(c), hipMemcpyDeviceToHost));
        std::fprintf(stderr, "[ctws] edt lower-envelope columns: y %u z %u\n", c[0], c[1]);
    }
    if (pl.pass2 && pl.nd_ws == 2) {
        // two_pass_watershed.py:139: no maxima on initial seeds; per-slice dt stats again
        k_p2_zero_dt<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.dt);
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)w.smin, 0xFFFFFFFFu, (size_t)TS, h->stream));
        HIPCHK(hipMemsetAsync(w.smax, 0, sizeof(uint32_t) * TS, h->stream));
        dim3 gs((unsigned)maxZ, nb);
        k_dt_slice_stats<<<gs, 256, 0, h->stream>>>(w.desc, w.stat, w.dt, w.smin, w.smax);
        LAUNCHCHK();
    }
    mark("edt_yz");

    // ---- seed map smoothing, hmap -----------------------------------------------------------
    HmapParams hp{(float)cfg->alpha, (float)(1.0 - cfg->alpha), pl.nd_ws == 2 ? 1 : 0};
    const float* seedmap = w.dt;
    if (pl.seeds_smooth) {
        bool any = false;
        for (int a = (pl.nd_ws == 3 ? 0 : 1); a < 3; ++a) any |= pl.sig_seeds[a] > 0.0;
        if (any) {
            if ((r = run_gauss(h, pl, pl.sig_seeds, false, w.dt, w.sm, nb, maxZ, maxY, maxX, hp, 0)) != CTWS_OK)
                return r;
            seedmap = w.sm;
        }
    }
    mark("smooth_seeds");
    {
        const double sw[3] = {pl.weights_smooth ? pl.sig_weights[0] : 0.0, pl.weights_smooth ? pl.sig_weights[1] : 0.0,
                              pl.weights_smooth ? pl.sig_weights[2] : 0.0};
        if ((r = run_gauss(h, pl, sw, true, w.fin, w.hm, nb, maxZ, maxY, maxX, hp, 1)) != CTWS_OK) return r;
    }
    mark("hmap");

    // ---- seeds: local maxima, plateaus, CC, vigra scan-order ids -----------------------------
    {
        HIPCHK(hipMemsetAsync(h->ptile.p, 0, sizeof(uint32_t) * (size_t)std::max<int64_t>(TPT, 1), h->stream));
        // k_localmax also writes the member bitmap, the strict maxima's forest entries and the
        // equal bitmap (in w.fopen: free until the flood), and the plateau kernels walk the
        // equal bitmap; the dense kernels read every class instead (CTWS_SEED_DENSE=1, and the
        // tile CC, which builds the member bitmap with atomicOr on a zeroed one)
        const bool dense = seed_dense;
        uint64_t* const feq = w.fopen;
        if (dense) k_localmax<<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, seedmap, w.cls, w.smax, (uint32_t*)h->ptile.p,
                                                         nullptr, nullptr, nullptr);
        else k_localmax<<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, seedmap, w.cls, w.smax, (uint32_t*)h->ptile.p,
                                                    w.fseed, feq, w.PF);
        LAUNCHCHK();
        // plateaus (equal-valued maxima candidates) and the seed CC: LDS tile union-find
        // (k_tilecc.hip); blocks without plateau voxels skip the plateau kernels on the device
        // the seed CC's member bitmap (CcArgs::troot for SEED): its parents are members-only
        if (dense) HIPCHK(hipMemsetAsync(w.fseed, 0, sizeof(uint64_t) * (size_t)TF, h->stream));
        CcArgs ca{seedmap, w.cls, w.P, nullptr, nullptr, 0, w.fseed, nullptr, (const uint32_t*)h->ptile.p};
        // one wave per 64 words of the equal bitmap
        const dim3 eg((unsigned)std::min<int64_t>((maxRows * ((maxX + 63) / 64) + 255) / 256, 2048), nb);
        if (pl.nd_ws == 3) {
            using T = CcTileM<3, CC_SEED>;  // (= the plateau tile)
            const dim3 tg(tiles8(cdiv(maxZ, T::TZ) * cdiv(maxY, T::TY) * cdiv(maxX, T::TX)), nb);
            k_tile_cc<3, CC_PLATEAU><<<tg, 256, 0, h->stream>>>(w.desc, w.stat, ca, w.P);
            k_tile_merge<3, CC_PLATEAU><<<dim3(std::min(tg.x, 2048u), tg.y), 256, 0, h->stream>>>(w.desc, w.stat, ca, w.P);
            if (dense) k_plateau_flag<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.cls, w.P);
            else k_plateau_flag_eq<<<eg, 256, 0, h->stream>>>(w.desc, w.stat, w.cls, w.P, feq);
            if (h->seed_tilecc) {
                k_tile_cc<3, CC_SEED><<<tg, 256, 0, h->stream>>>(w.desc, w.stat, ca, w.PF);
                k_tile_merge<3, CC_SEED><<<dim3(std::min(tg.x, 2048u), tg.y), 256, 0, h->stream>>>(w.desc, w.stat, ca, w.PF);
            } else if (dense) {
                // the seed components are the maximal plateaus and the isolated maxima (k_cc.hip)
                k_seed_members<3><<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, w.cls, w.P, w.PF, w.fseed, nullptr);
            } else {
                k_seed_members_eq<3><<<eg, 256, 0, h->stream>>>(w.desc, w.stat, w.cls, w.P, w.PF, w.fseed, feq, nullptr);
            }
        } else {
            using T = CcTile<2>;
            const dim3 tg(tiles8(cdiv(maxZ, T::TZ) * cdiv(maxY, T::TY) * cdiv(maxX, T::TX)), nb);
            k_tile_cc<2, CC_PLATEAU><<<tg, 256, 0, h->stream>>>(w.desc, w.stat, ca, w.P);
            k_tile_merge<2, CC_PLATEAU><<<dim3(std::min(tg.x, 2048u), tg.y), 256, 0, h->stream>>>(w.desc, w.stat, ca, w.P);
            if (dense) k_plateau_flag<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.cls, w.P);
            else k_plateau_flag_eq<<<eg, 256, 0, h->stream>>>(w.desc, w.stat, w.cls, w.P, feq);
            if (h->seed_tilecc) {
                k_tile_cc<2, CC_SEED><<<tg, 256, 0, h->stream>>>(w.desc, w.stat, ca, w.PF);
                k_tile_merge<2, CC_SEED><<<dim3(std::min(tg.x, 2048u), tg.y), 256, 0, h->stream>>>(w.desc, w.stat, ca, w.PF);
            } else {
                // every maximum its own root; the plateau maxima listed (in w.A, free until the size
                // filter) and united with their 4-adjacent maxima (k_cc.hip)
                if (dense)
                    k_seed_members<2><<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, w.cls, w.P, w.PF, w.fseed,
                                                                 (uint32_t*)w.A);
                else
                    k_seed_members_eq<2><<<eg, 256, 0, h->stream>>>(w.desc, w.stat, w.cls, w.P, w.PF, w.fseed, feq,
                                                                   (uint32_t*)w.A);
                k_seed_union2<<<dim3(64, nb), 256, 0, h->stream>>>(w.desc, w.stat, w.cls, w.P, (const uint32_t*)w.A,
                                                                   w.PF);
            }
        }
        LAUNCHCHK();
    }
    HIPCHK(hipMemsetAsync(w.W, 0, sizeof(uint64_t) * (size_t)TW, h->stream));
    k_flatten_seeds<<<dim3((unsigned)std::min<int64_t>((TF / nb + 255) / 256 + 1, 4096), nb), 256, 0, h->stream>>>(
        w.desc, w.stat, w.PF, w.fseed, w.W);
    k_bitmap_csum<<<wg, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.W, w.csum);
    k_chunk_scan<<<nb, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.csum, 0);
    k_word_prefix<<<wg, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.W, w.csum, w.Wp);
    // (pass 1: the roots' positions per label for the sparse size filter, in w.Bf -- free after
    // the hmap; pass 2 relabels the seeds and records its ids' first positions below)
    k_root_label<<<wg, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.PF, w.W, w.Wp, pl.pass2 ? nullptr : (uint32_t*)w.Bf);
    if (pl.pass2) {
        // _apply_watershed_with_seeds: shifted seeds + initial seeds, relabelConsecutive
        // the slices' seed bases of the seed CC into w.soff (free until k_slice_offsets): the
        // relabel keys of 2-D blocks need them after w.sb is rewritten for the new ids
        k_slice_seed_base<<<gsb, 256, 0, h->stream>>>(w.desc, w.stat, w.W, w.Wp, w.soff);
        HIPCHK(hipMemsetAsync(w.hkey, 0xFF, sizeof(uint64_t) * (size_t)TH, h->stream));
        HIPCHK(hipMemsetAsync(w.hpos, 0xFF, sizeof(uint32_t) * (size_t)TH, h->stream));
        // the relabel key of a voxel is computed where it is read (p2_value), no key array in HBM
        k_p2_insert<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.hkey, w.hpos, w.PF, w.fseed, w.soff,
                                               (const uint32_t*)h->p2_hint_dev.p);
        HIPCHK(hipMemsetAsync(w.W, 0, sizeof(uint64_t) * (size_t)TW, h->stream));
        const dim3 hg((unsigned)std::min<int64_t>((maxH + 255) / 256, 4096), nb);
        k_p2_roots<<<hg, 256, 0, h->stream>>>(w.desc, w.stat, w.hkey, w.hpos, w.W);
        k_bitmap_csum<<<wg, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.W, w.csum);
        k_chunk_scan<<<nb, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.csum, 0);
        k_word_prefix<<<wg, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.W, w.csum, w.Wp);
        // the first position of each new id (a seed: it keeps the id) for the sparse size
        // filter, in w.dt (free after the seed CC)
        k_root_label<<<wg, 256, 0, h->stream>>>(w.desc, w.stat, 0, nullptr, w.W, w.Wp, (uint32_t*)w.dt);
        LAUNCHCHK();
    }
    }  // !from_seeds
    // packed flood keys need labels < 2^20 in every block of the batch
    {
        HIPCHK(hipMemcpyAsync(s2.data(), w.stat, sizeof(BlockStat) * nb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (auto& s : s2) {
            // (WatershedFromSeeds: a seedless block's seeds are its n_auto strict minima)
            const uint32_t ns = std::max(s.n_seeds, pl.from_seeds ? s.n_auto : 0u);
            if (ns >= (1u << 20) - 1u) packed = false;
            max_seeds = std::max(max_seeds, ns);
        }
        if (h->force_wide || h->wide_rerun) packed = false;
        if (!packed) {
            set_tiles(false);
            HIPCHK(hipMemcpyAsync(w.desc, desc.data(), sizeof(BlockDesc) * nb, hipMemcpyHostToDevice, h->stream));
            h->last_desc = desc;
        }
    }
    uint8_t* excl = nullptr;
    const bool descent = packed && !h->no_descent;
    const bool cc_seeds = descent && !pl.pass2 && !pl.from_seeds && h->stop_after != CTWS_STOP_SEEDS;
    const uint32_t* cc = cc_seeds ? w.PF : nullptr;
    if (pl.pass2) {
        k_slice_seed_base<<<gsb, 256, 0, h->stream>>>(w.desc, w.stat, w.W, w.Wp, w.sb);
        excl = (uint8_t*)w.fin;  // free after the hmap
        k_p2_excl_zero<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, excl);
        // 3-D: k_p2_label marks the exclusions from the initial values it reads anyway
        const int fused3 = pl.nd_ws == 3 ? 1 : 0;
        k_p2_label<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.hkey, w.hpos, w.W, w.Wp, w.hm, w.lab, w.key, w.cls,
                                              (uint32_t*)w.Bf, (uint32_t*)w.sm, packed ? 1 : 0, descent ? 0 : 1, w.PF,
                                              w.fseed, w.soff, (const uint32_t*)h->p2_hint_dev.p,
                                              fused3 ? excl : nullptr);
        if (!fused3) k_p2_excl<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.sb, excl);
    } else if (pl.from_seeds) {
        // labels, keys and seed flags in the packed / wide key form (fs_seeds counted them)
        if (pl.sf_fill)
            k_fs_label<uint64_t><<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.hkey, w.hpos, w.hm, w.lab, w.key, w.cls,
                                                            packed ? 1 : 0);
        else
            k_fs_label<uint32_t><<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.hkey, w.hpos, w.hm, w.lab, w.key, w.cls,
                                                            packed ? 1 : 0);
        k_fs_auto_label<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.surv, w.W, w.Wp, w.hm, w.lab, w.key, w.cls,
                                                   packed ? 1 : 0);
    } else {
        // the descent flood reads the seeds from the CC parents directly (cc_seeds)
        if (!cc_seeds)
            k_seed_label<<<rg, 256, 0, h->stream>>>(w.desc, w.stat, w.PF, w.fseed, w.hm, w.lab, w.key, w.cls,
                                                    packed ? 1 : 0);
        k_slice_seed_base<<<gsb, 256, 0, h->stream>>>(w.desc, w.stat, w.W, w.Wp, w.sb);
    }
    LAUNCHCHK();
    mark("seeds");
    if (h->stop_after == CTWS_STOP_SEEDS) {
        HIPCHK(hipStreamSynchronize(h->stream));
        return CTWS_OK;
    }

    // ---- flood ------------------------------------------------------------------------------
    int rounds1 = 0, rounds2 = 0;
    h->flood_tiles = h->flood_iters = h->flood_lines = 0;
    float fk1 = 0.f, fk2 = 0.f;
    int fallback = 0, fiters = 0, fiters2 = 0;
    // statistics (CTWS_TRACE only): open voxels and frontier visits per block
    uint32_t* fst = h->trace ? w.fstat : nullptr;
    // 2-D ws, pass 1: the first flood's fixpoint check counts the labels for the size filter as it
    // reads the keys (k_flood_verify_hist2d).  Every other path counts with k_hist2d / k_hist
    // below: wide keys, pass 2, WatershedFromSeeds, 3-D ws, a stop after the flood, and a batch
    // flooded again after a violation (its counts would be stale).
    uint32_t* const counts = (uint32_t*)w.A;  // (w.A: free from the seed CC to the size filter)
    const bool fuse_hist = h->fuse_hist && descent && pl.nd_ws == 2 && !pl.pass2 && !pl.from_seeds &&
                           cfg->size_filter > 0 && h->stop_after != CTWS_STOP_FLOOD;
    bool counts_ready = false;
    if (descent) {
        // descent pre-pass (k_flood.hip): voxels whose steepest descent reaches a seed are final
        // tile-local descent + pointer jumping (16^3 / 1 x 64 x 64 tiles)
        const int dz = pl.nd_ws == 3 ? 16 : 1, dy = pl.nd_ws == 3 ? 16 : 64, dx = pl.nd_ws == 3 ? 16 : 64;  // DTile
        const dim3 dg(tiles8(((maxZ + dz - 1) / dz) * ((maxY + dy - 1) / dy) * ((maxX + dx - 1) / dx)), nb);
        {
            if (pl.nd_ws == 3) k_descent_tile<3><<<dg, 512, 0, h->stream>>>(w.desc, w.stat, w.hm, w.lab, cc, w.fseed, w.P);
            else k_descent_tile<2><<<dg, 512, 0, h->stream>>>(w.desc, w.stat, w.hm, w.lab, cc, w.fseed, w.P);
            LAUNCHCHK();
        }
        mark("descent_tile");
        if (fst) HIPCHK(hipMemsetAsync(fst, 0, sizeof(uint32_t) * 2 * (size_t)nb, h->stream));
        // masked blocks: their plateau leaves the open set until the rest is flooded (k_plateau.hip);
        // the plateau level comes out of the descent pass
        bool any_mask = false;
        for (int i = 0; i < nb; ++i) any_mask |= desc[i].mask != nullptr;
        const bool plat_fill = h->plateau_fill && packed && any_mask;
        if (plat_fill) HIPCHK(hipMemsetAsync(w.plev, 0, sizeof(uint32_t) * (size_t)nb, h->stream));
        // 8 words in flight per wave step (4: +0.1 ms on config 3, +0.6 ms on config 4)
        k_descent_init<8><<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.P, w.key, w.cls, w.fopen,
                                                     w.front0, fst, plat_fill ? w.plev : nullptr);
        LAUNCHCHK();
        if (plat_fill) {
            HIPCHK(hipMemsetAsync(w.fplat, 0, sizeof(uint64_t) * (size_t)TF, h->stream));
            k_plat_mark<<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.plev, w.fopen, w.fplat);
            LAUNCHCHK();
        }
        mark("flood_descent");
        // the remaining voxels: the frontier relaxation (k_frontier, one voxel per lane)
        if ((r = run_frontier(h, pl, nb, TF, max_tiles, TT, packed, fst, &fiters, &rounds1, &fk1)) != CTWS_OK)
            return r;
        if (plat_fill) {
            // the plateau: entries, min-plus runs along x, y (, z), then the frontier from there
            if (pl.nd_ws == 3) k_plat_entry<3><<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.key, w.fplat, w.plev);
            else k_plat_entry<2><<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.key, w.fplat, w.plev);
            const unsigned rows_g = (unsigned)std::min<int64_t>(((int64_t)maxZ * maxY + 3) / 4, 4096);
            const unsigned cols_g = (unsigned)std::min<int64_t>(((int64_t)std::max(maxZ, maxY) * ((maxX + 63) / 64) + 3) / 4, 4096);
            k_plat_scan_x<<<dim3(rows_g, nb), 256, 0, h->stream>>>(w.desc, w.stat, w.key, w.fplat, w.plev);
            k_plat_scan_col<1><<<dim3(cols_g, nb), 256, 0, h->stream>>>(w.desc, w.stat, w.key, w.fplat, w.plev);
            if (pl.nd_ws == 3)
                k_plat_scan_col<2><<<dim3(cols_g, nb), 256, 0, h->stream>>>(w.desc, w.stat, w.key, w.fplat, w.plev);
            k_plat_restore<<<dim3((unsigned)std::min<int64_t>(((int64_t)maxZ * maxY * ((maxX + 63) / 64) + 255) / 256, 4096), nb), 256, 0, h->stream>>>(w.desc, w.stat, w.fopen, w.fplat,
                                                                                  w.front0);
            LAUNCHCHK();
            if ((r = run_frontier(h, pl, nb, TF, max_tiles, TT, packed, fst, &fiters, &rounds1, &fk1)) != CTWS_OK)
                return r;
        }
        mark("flood_relax");
        if (fst) {
            std::vector<uint32_t> hs(2 * (size_t)nb);
            HIPCHK(hipMemcpyAsync(hs.data(), fst, sizeof(uint32_t) * 2 * (size_t)nb, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            double no = 0, nv = 0;
            for (int i = 0; i < nb; ++i) {
                no += hs[i];
                nv += hs[nb + i];
            }
            add_timing(h, "open_voxels", (float)no);
            add_timing(h, "frontier_visits", (float)nv);
        }
        // fixpoint check of every voxel the relaxation solved (a guard: the descent argument and
        // the frontier's convergence make a violation impossible; on a violation the batch is
        // flooded again from the seeds alone) and the d-saturation detector (a solved key with d
        // at kDMax sets BlockStat::dsat: the block runs again on the wide keys).  The kernel
        // always runs; CTWS_VERIFY=0 drops only the violation handling.
        HIPCHK(hipMemsetAsync(w.counter, 0, 40, h->stream));
        if (fuse_hist) {
            k_hist_zero<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, counts);
            // LDS bins: the power of two above 1.5 x the labels per slice of the batch's densest
            // block (a slice with more labels counts with global atomics)
            int64_t per_slice = 0;
            for (int i = 0; i < nb; ++i)
                if (s2[i].active) per_slice = std::max<int64_t>(per_slice, (int64_t)s2[i].n_seeds / std::max(desc[i].Z, 1) + 1);
            int bins = 512;
            while (bins < kHist2dBins && bins < per_slice + per_slice / 2) bins *= 2;
            k_flood_verify_hist2d<<<dim3((unsigned)maxZ * 4, nb), kVerifyHistThreads, sizeof(uint32_t) * (size_t)bins,
                                    h->stream>>>(w.desc, w.stat, w.hm, w.key, w.fopen, w.sb, counts, w.counter, 4, bins);
            counts_ready = true;
        } else if (pl.nd_ws == 3)
            k_flood_verify<3><<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.key, w.fopen, w.counter);
        else
            k_flood_verify<2><<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.key, w.fopen, w.counter);
        LAUNCHCHK();
        if (h->verify) {
            HIPCHK(hipMemcpyAsync(h->h_counter, w.counter, 40, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            if (h->trace && h->h_counter[0]) {
                fprintf(stderr, "[ctws] flood verify: violations at");
                for (uint32_t k = 0; k < std::min(8u, h->h_counter[1]); ++k) fprintf(stderr, " %u", h->h_counter[2 + k]);
                fprintf(stderr, "\n");
            }
            if (h->h_counter[0] && h->verify >= 2) {
                h->err = "flood fixpoint check failed (CTWS_VERIFY=2)";
                return CTWS_EHIP;
            }
            if (h->h_counter[0] && !h->no_fallback) {
                fallback = 1;
                counts_ready = false;  // the keys change: the size filter counts again
                k_flood_reset<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.lab, cc, w.fseed, w.key, w.cls);
                LAUNCHCHK();
                if ((r = run_flood(h, pl.nd_ws, packed, nb, max_tiles, TT, w.hm, false, &rounds1, &fk1)) != CTWS_OK)
                    return r;
            }
        }
        mark("flood_verify");
    } else {
        mark("flood_descent");
        if ((r = run_flood(h, pl.nd_ws, packed, nb, max_tiles, TT, w.hm, false, &rounds1, &fk1)) != CTWS_OK) return r;
    }
    // test hooks that stop after the flood read the workspace: a batch with a saturated packed
    // key (note_dsat) is run again whole on the wide keys, so they see the unbounded fixpoint too
    bool rerun_done = false;
    auto stop_dsat = [&]() -> int {
        if (!packed) return CTWS_OK;
        std::vector<BlockStat> sd(nb);
        HIPCHK(hipMemcpyAsync(sd.data(), w.stat, sizeof(BlockStat) * nb, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        bool any = false;
        for (auto& x : sd) any |= x.active && x.dsat;
        if (!any) return CTWS_OK;
        ++h->wide_rerun;
        const int rr = run_batch(h, cfg, pl, blocks, io, nb);
        --h->wide_rerun;
        rerun_done = true;
        return rr;
    };
    if (h->stop_after == CTWS_STOP_FLOOD) {
        if ((r = stop_dsat()) != CTWS_OK || rerun_done) return r;
    }
    // the histogram, the filter and (pass 1) the final labels read the packed keys directly
    // (pass 2 reads its final labels from the packed keys too: k_slice_max, k_p2_output)
    if (packed && h->stop_after == CTWS_STOP_FLOOD)
        k_unpack_labels<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.key, w.lab);
    mark("flood");
    if (h->stop_after == CTWS_STOP_FLOOD) {
        HIPCHK(hipStreamSynchronize(h->stream));
        return CTWS_OK;
    }

    // ---- size filter + regrow ---------------------------------------------------------------
    std::vector<uint32_t> surv(TS, 1u);
    int n_auto_blocks = 0;
    int n_sf_sparse = 0, n_sf_redo = 0;  // blocks whose removed segments were walked / walked, then scanned
    bool regrow_bad = false;  // the regrow's fixpoint check failed: the batch's blocks fail
    if (cfg->size_filter > 0) {
        auto histogram = [&]() -> int {
            k_hist_zero<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, counts);
            if (pl.nd_ws == 2) {
                // one LDS histogram per slice quarter over the slice's label range
                const dim3 g2((unsigned)maxZ * 4, nb);
                if (packed) k_hist2d<1><<<g2, 256, 0, h->stream>>>(w.desc, w.stat, w.lab, w.key, w.sb, counts, 4);
                else k_hist2d<0><<<g2, 256, 0, h->stream>>>(w.desc, w.stat, w.lab, w.key, w.sb, counts, 4);
            } else {
                // 32K voxels per workgroup: the LDS histogram is cleared / flushed once per 128 voxels
                dim3 hg((unsigned)std::min<int64_t>((maxN + 32767) / 32768, 2048), nb);
                const int bins = (int64_t)max_seeds + 1 <= kHistBins ? (int)max_seeds + 1 : 0;
                const size_t lds = sizeof(uint32_t) * (size_t)bins;
                if (packed) k_hist<1><<<hg, 256, lds, h->stream>>>(w.desc, w.stat, w.lab, w.key, counts, bins);
                else k_hist<0><<<hg, 256, lds, h->stream>>>(w.desc, w.stat, w.lab, w.key, counts, bins);
            }
            LAUNCHCHK();
            return CTWS_OK;
        };
        if (!counts_ready && (r = histogram()) != CTWS_OK) return r;
        if (packed) {
            // survivors -> regrow seeds, removed voxels -> open; then the frontier relaxation
            std::vector<BlockStat> s3(nb);
            // a small size filter: the removed segments walked from their seeds (k_sf_plan decides
            // per block; CTWS_SF_SPARSE=0 scans every block).  WatershedFromSeeds numbers its
            // labels by seed value, without first positions: it scans.  A pass-2 label is every
            // voxel that carried one initial id, in several pieces where the outer block or a 2-D
            // slice cut a pass-1 segment: a walk that reaches fewer voxels than its label counts
            // hands its block back to the scan below (BlockStat::sf_redo)
            const bool sparse_ok = h->sf_sparse && !pl.from_seeds && cfg->size_filter <= 64;
            const uint32_t* rootpos = pl.pass2 ? (const uint32_t*)w.dt : (const uint32_t*)w.Bf;
            auto regrow_init = [&]() -> int {
                HIPCHK(hipMemsetAsync(w.surv, 0, sizeof(uint32_t) * TS, h->stream));
                if (sparse_ok) {
                    const unsigned split = std::min<unsigned>(kSfPlanSplit, max_seeds / kSfPlanLabels + 1);
                    k_sf_plan<<<dim3(split, nb), 256, 0, h->stream>>>(
                        w.desc, w.stat, (uint32_t)cfg->size_filter, counts, excl, w.sb, w.surv, w.sfacc);
                    HIPCHK(hipMemsetAsync(w.fopen, 0, sizeof(uint64_t) * (size_t)TF, h->stream));
                    HIPCHK(hipMemsetAsync(w.front0, 0, sizeof(uint64_t) * (size_t)TF, h->stream));
                    k_sf_sparse<<<dim3((unsigned)std::max<uint32_t>((max_seeds + 255) / 256, 1u), nb), 256, 0,
                                   h->stream>>>(w.desc, w.stat, (uint32_t)cfg->size_filter, counts, excl,
                                                rootpos, w.hm, w.key, w.cls, w.fopen, w.front0);
                    LAUNCHCHK();
                }
                // 4 words per wave step (8: +1.2 ms on config 3, +2.2 ms on config 4)
                k_regrow_init<4><<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, (uint32_t)cfg->size_filter, counts,
                                                            excl, w.hm, w.key, w.cls, w.fopen, w.front0, w.surv);
                LAUNCHCHK();
                HIPCHK(hipMemcpyAsync(surv.data(), w.surv, sizeof(uint32_t) * TS, hipMemcpyDeviceToHost, h->stream));
                HIPCHK(hipMemcpyAsync(s3.data(), w.stat, sizeof(BlockStat) * nb, hipMemcpyDeviceToHost, h->stream));
                HIPCHK(hipStreamSynchronize(h->stream));
                return CTWS_OK;
            };
            if ((r = regrow_init()) != CTWS_OK) return r;
            for (int i = 0; i < nb; ++i) {
                if (!s3[i].active) continue;
                const int ns = pl.nd_ws == 2 ? desc[i].Z : 1;
                bool need = false;
                for (int z = 0; z < ns; ++z) need |= !surv[desc[i].sbase + z];
                n_auto_blocks += need;
                n_sf_sparse += sparse_ok && s3[i].sf_sparse;
                n_sf_redo += sparse_ok && s3[i].sf_redo;
            }
            if (n_auto_blocks) {
                // every segment of a slice / block removed: vigra seeds the regrow from the strict
                // local minima of the hmap (watershedsNew with an all-zero seed image)
                HIPCHK(hipMemsetAsync(w.W, 0, sizeof(uint64_t) * (size_t)TW, h->stream));
                const dim3 ag((unsigned)std::min<int64_t>(maxRows, 65535), nb);
                k_auto_minima<<<ag, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.surv, w.W);
                k_bitmap_csum<<<wg, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.W, w.csum);
                k_chunk_scan<<<nb, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.csum, 2);
                k_word_prefix<<<wg, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.W, w.csum, w.Wp);
                k_auto_seed_set<<<ag, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.surv, w.W, w.Wp, w.sb, w.key,
                                                           w.cls, w.fopen, w.front0, nullptr);
                LAUNCHCHK();
            }
            if ((r = run_frontier(h, pl, nb, TF, max_tiles, TT, packed, nullptr, &fiters2, &rounds2, &fk2, true)) !=
                CTWS_OK)
                return r;
            // the regrow's fixpoint at the voxels it solved (the removed ones), and its d
            // saturation (as after the first flood: the kernel always runs)
            HIPCHK(hipMemsetAsync(w.counter, 0, 40, h->stream));
            if (pl.nd_ws == 3)
                k_flood_verify<3><<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.key, w.fopen, w.counter);
            else
                k_flood_verify<2><<<wtg, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.key, w.fopen, w.counter);
            LAUNCHCHK();
            if (h->verify) {
                HIPCHK(hipMemcpyAsync(h->h_counter, w.counter, 40, hipMemcpyDeviceToHost, h->stream));
                HIPCHK(hipStreamSynchronize(h->stream));
                if (h->h_counter[0] && h->verify >= 2) {
                    h->err = "regrow fixpoint check failed (CTWS_VERIFY=2)";
                    return CTWS_EHIP;
                }
                regrow_bad = h->h_counter[0] != 0;
            }
        } else {
            FilterParams fp{(uint32_t)cfg->size_filter, 0, 0, 0, w.act0};
            flood_tile_dims(pl.nd_ws, packed, &fp.tz, &fp.ty, &fp.tx);
            HIPCHK(hipMemsetAsync(w.act0, 0, sizeof(uint32_t) * (size_t)TT, h->stream));
            HIPCHK(hipMemsetAsync(w.surv, 0, sizeof(uint32_t) * TS, h->stream));
            k_size_filter<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, fp, counts, excl, w.hm, w.lab, w.key, w.cls,
                                                     w.surv, packed ? 1 : 0);
            LAUNCHCHK();
            HIPCHK(hipMemcpyAsync(surv.data(), w.surv, sizeof(uint32_t) * TS, hipMemcpyDeviceToHost, h->stream));
            std::vector<BlockStat> s3(nb);
            HIPCHK(hipMemcpyAsync(s3.data(), w.stat, sizeof(BlockStat) * nb, hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            for (int i = 0; i < nb; ++i) {
                if (!s3[i].active) continue;
                const int ns = pl.nd_ws == 2 ? desc[i].Z : 1;
                bool need = false;
                for (int z = 0; z < ns; ++z) need |= !surv[desc[i].sbase + z];
                n_auto_blocks += need;
            }
            if (n_auto_blocks) {
                // vigra's auto-seeding (above) on the wide keys: the strict minima as fixed seeds
                // with their labels in lab (any width); their tiles were freed, so they are active
                HIPCHK(hipMemsetAsync(w.W, 0, sizeof(uint64_t) * (size_t)TW, h->stream));
                const dim3 ag((unsigned)std::min<int64_t>(maxRows, 65535), nb);
                k_auto_minima<<<ag, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.surv, w.W);
                k_bitmap_csum<<<wg, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.W, w.csum);
                k_chunk_scan<<<nb, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.csum, 2);
                k_word_prefix<<<wg, 256, 0, h->stream>>>(w.desc, w.stat, 0, w.W, w.csum, w.Wp);
                k_auto_seed_set<<<ag, 256, 0, h->stream>>>(w.desc, w.stat, w.hm, w.surv, w.W, w.Wp, w.sb, w.key,
                                                           w.cls, nullptr, nullptr, w.lab);
                LAUNCHCHK();
            }
            if ((r = run_flood(h, pl.nd_ws, packed, nb, max_tiles, TT, w.hm, true, &rounds2, &fk2)) != CTWS_OK)
                return r;
        }
    }
    mark("size_filter");
    const int keys_final = packed ? 1 : 0;  // final labels still in the keys

    // ---- pass 2: per-slice offsets, takeDict, uncropped inner write --------------------------
    const int ssplit = 4;  // workgroups per slice of the per-slice reductions
    if (pl.pass2) {
        if (pl.nd_ws == 2) {
            k_slice_max<<<dim3((unsigned)maxZ * ssplit, nb), 256, 0, h->stream>>>(w.desc, w.stat, w.lab, w.key,
                                                                                  keys_final, w.sb, w.slmax, ssplit, 1);
            k_slice_offsets<<<nb, 64, 0, h->stream>>>(w.desc, w.stat, w.slmax, w.soff);
            k_p2_check<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.hkey, w.soff);
        }
        // per slice: an in-mask voxel (2-D only: a seedless 3-D block fails whatever its mask)
        HIPCHK(hipMemsetAsync(w.smin, 0, sizeof(uint32_t) * TS, h->stream));  // free after the hmap
        if (pl.nd_ws == 2) k_slice_inmask<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.smin);
        mark("finalize");
        mark("crop_cc");
        k_p2_output<<<ig, 256, 0, h->stream>>>(w.desc, w.stat, w.lab, w.key, keys_final, (const uint32_t*)w.Bf,
                                               (const uint32_t*)w.sm, w.soff);
        LAUNCHCHK();
        mark("output");
    } else if (pl.from_seeds) {
        // WatershedFromSeeds: labels -> seed values (uint64), masked voxels 0; no crop / offset
        mark("finalize");
        mark("crop_cc");
        if (pl.sf_fill)
            k_fs_output<uint64_t><<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.lab, w.key, keys_final,
                                                             (const uint64_t*)h->fs_sorted.p, w.surv,
                                                             cfg->size_filter > 0 ? 1 : 0);
        else
            k_fs_output<uint32_t><<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.lab, w.key, keys_final,
                                                             (const uint32_t*)h->fs_sorted.p, w.surv,
                                                             cfg->size_filter > 0 ? 1 : 0);
        LAUNCHCHK();
        mark("output");
    } else {
        // ---- 2-D offsets (uncropped blocks only: a cropped block is renumbered by its CC) ----
        bool any_crop = false, any_plain2d = false;
        for (int i = 0; i < nb; ++i) {
            any_crop |= desc[i].crop != 0;
            any_plain2d |= desc[i].crop == 0 && pl.nd_ws == 2;
        }
        const bool stop_ws = h->stop_after == CTWS_STOP_WS;
        if (pl.nd_ws == 2 && (any_plain2d || stop_ws)) {
            k_slice_max<<<dim3((unsigned)maxZ * ssplit, nb), 256, 0, h->stream>>>(
                w.desc, w.stat, w.lab, w.key, keys_final, w.sb, w.slmax, ssplit, stop_ws ? 1 : 0);
            k_slice_offsets<<<nb, 64, 0, h->stream>>>(w.desc, w.stat, w.slmax, w.soff);
        }
        if (stop_ws) {
            if ((r = stop_dsat()) != CTWS_OK || rerun_done) return r;
            // test hook: the final uint32 ws of the outer block in `lab`
            k_finalize_ws<<<vg, 256, 0, h->stream>>>(w.desc, w.stat, w.sb, w.soff, w.key, keys_final, w.lab);
            LAUNCHCHK();
            HIPCHK(hipStreamSynchronize(h->stream));
            return CTWS_OK;
        }
        LAUNCHCHK();
        mark("finalize");

        // ---- halo crop CC (labelVolumeWithBackground) + uint64 output --------------------------
        if (any_crop) {
            // tile roots of the crop CC marked in the (free) frontier bitmap front0
            HIPCHK(hipMemsetAsync(w.front0, 0, sizeof(uint64_t) * (size_t)TF, h->stream));
            CcArgs ca{nullptr, nullptr, nullptr, w.lab, w.key, keys_final, w.front0, (uint64_t*)h->xface.p, nullptr};
            const dim3 wgi((unsigned)((words_of(maxNI) + 255) / 256), nb);
            if (pl.nd_ws == 3) {
                using T = CcTile<3>;
                const dim3 tg(tiles8(cdiv(maxIZ, T::TZ) * cdiv(maxIY, T::TY) * cdiv(maxIX, T::TX)), nb);
                k_tile_cc<3, CC_CROP><<<tg, 256, 0, h->stream>>>(w.desc, w.stat, ca, w.PF);
                k_tile_merge<3, CC_CROP><<<dim3(std::min(tg.x, 2048u), tg.y), 256, 0, h->stream>>>(w.desc, w.stat, ca, w.PF);
            } else {
                using T = CcTile<2>;
                const dim3 tg(tiles8(cdiv(maxIZ, T::TZ) * cdiv(maxIY, T::TY) * cdiv(maxIX, T::TX)), nb);
                k_tile_cc<2, CC_CROP><<<tg, 256, 0, h->stream>>>(w.desc, w.stat, ca, w.PF);
                k_tile_merge<2, CC_CROP><<<dim3(std::min(tg.x, 2048u), tg.y), 256, 0, h->stream>>>(w.desc, w.stat, ca, w.PF);
            }
            HIPCHK(hipMemsetAsync(w.W, 0, sizeof(uint64_t) * (size_t)TW, h->stream));
            k_flatten_tile_roots<<<wgi, 256, 0, h->stream>>>(w.desc, w.stat, w.PF, w.front0, w.W);
            k_bitmap_csum<<<wgi, 256, 0, h->stream>>>(w.desc, w.stat, 1, w.W, w.csum);
            k_chunk_scan<<<nb, 256, 0, h->stream>>>(w.desc, w.stat, 1, w.csum, 1);
            k_word_prefix<<<wgi, 256, 0, h->stream>>>(w.desc, w.stat, 1, w.W, w.csum, w.Wp);
            k_root_label<<<wgi, 256, 0, h->stream>>>(w.desc, w.stat, 1, w.PF, w.W, w.Wp, nullptr);
            LAUNCHCHK();
        }
        mark("crop_cc");
        bool any_plain = false;
        for (int i = 0; i < nb; ++i) any_plain |= desc[i].crop == 0;
        // uncropped blocks count their distinct ids in W (cropped blocks: n_cc of the crop CC)
        if (any_plain) HIPCHK(hipMemsetAsync(w.W, 0, sizeof(uint64_t) * (size_t)TW, h->stream));
        // cropped blocks: one workgroup per crop-CC tile, labels through LDS (k_output_crop)
        const bool crop_tiles = any_crop && h->output_tile;
        // (k_output still writes the uncropped blocks and the empty ones: constant offset)
        k_output<<<wtig, 256, 0, h->stream>>>(w.desc, w.stat, w.lab, w.key, keys_final, w.PF, w.sb, w.soff,
                                             (unsigned long long*)w.W, crop_tiles ? 1 : 0);
        if (crop_tiles) {
            if (pl.nd_ws == 3) {
                using T = CcTile<3>;
                const dim3 tg(tiles8(cdiv(maxIZ, T::TZ) * cdiv(maxIY, T::TY) * cdiv(maxIX, T::TX)), nb);
                k_output_crop<3><<<tg, 256, 0, h->stream>>>(w.desc, w.stat, w.PF, w.front0);
            } else {
                using T = CcTile<2>;
                const dim3 tg(tiles8(cdiv(maxIZ, T::TZ) * cdiv(maxIY, T::TY) * cdiv(maxIX, T::TX)), nb);
                k_output_crop<2><<<tg, 256, 0, h->stream>>>(w.desc, w.stat, w.PF, w.front0);
            }
        }
        if (any_plain) k_count_ids<<<dim3(64, nb), 256, 0, h->stream>>>(w.desc, w.stat, w.W);
        LAUNCHCHK();
        mark("output");
    }

    HIPCHK(hipMemcpyAsync(st.data(), w.stat, sizeof(BlockStat) * nb, hipMemcpyDeviceToHost, h->stream));
    std::vector<uint32_t> sbh, inmask, soffh;
    if (pl.pass2) {
        sbh.resize(TS);
        inmask.resize(TS);
        HIPCHK(hipMemcpyAsync(sbh.data(), w.sb, sizeof(uint32_t) * TS, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(inmask.data(), w.smin, sizeof(uint32_t) * TS, hipMemcpyDeviceToHost, h->stream));
        if (pl.nd_ws == 2) {
            soffh.resize(TS);
            HIPCHK(hipMemcpyAsync(soffh.data(), w.soff, sizeof(uint32_t) * TS, hipMemcpyDeviceToHost, h->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = 1; i < ev; ++i) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, h->events[i - 1], h->events[i]);
        add_timing(h, names[i], ms);
    }
    add_timing(h, "flood_rounds", (float)rounds1);
    add_timing(h, "frontier_iters", (float)fiters);
    add_timing(h, "regrow_iters", (float)fiters2);
    add_timing(h, "flood_fallback", (float)fallback);
    add_timing(h, "regrow_rounds", (float)rounds2);
    add_timing(h, "auto_seeded_blocks", (float)n_auto_blocks);
    add_timing(h, "sf_sparse_blocks", (float)n_sf_sparse);
    add_timing(h, "sf_redo_blocks", (float)n_sf_redo);
    add_timing(h, "hist_fused", counts_ready ? 1.f : 0.f);  // batches whose flood check counted the labels
    // batches whose seed stage read every class byte again (CTWS_SEED_DENSE=1, CTWS_SEED_TILECC=1)
    add_timing(h, "seed_dense", seed_dense ? 1.f : 0.f);
    add_timing(h, "flood_kernel_ms", fk1);
    add_timing(h, "flood_packed", packed ? 1.f : 0.f);
    add_timing(h, "flood_tiles_solved", (float)h->flood_tiles);
    add_timing(h, "flood_local_iters", (float)h->flood_iters);
    add_timing(h, "flood_lines_swept", (float)h->flood_lines);
    add_timing(h, "size_filter_kernel_ms", fk2);
    // blocks whose packed flood ended with a key with d at kDMax (note_dsat): the 12-bit hop distance
    // may have saturated, so they are flooded again on the wide keys (32-bit d) below, never
    // returned with a possibly different fixpoint
    std::vector<int> wide;
    if (packed)
        for (int i = 0; i < nb; ++i)
            if (st[i].active && st[i].dsat) wide.push_back(i);
    auto in_wide = [&](int i) { return std::find(wide.begin(), wide.end(), i) != wide.end(); };
    // pass 2 (2-D): blocks whose relabel needs the wrapped-id merge (k_p2_check) or whose offsets
    // differ from the hint they ran with run again with their offsets as the hint
    std::vector<int> redo;
    std::vector<std::vector<uint32_t>> redo_hint;
    if (pl.pass2 && pl.nd_ws == 2) {
        for (int i = 0; i < nb; ++i) {
            if (!st[i].active || in_wide(i)) continue;
            std::vector<uint32_t> so(soffh.begin() + desc[i].sbase, soffh.begin() + desc[i].sbase + desc[i].Z);
            const bool again = desc[i].p2hint < 0 ? (st[i].err & kErrCollision) != 0 : so != h->p2_hints[i];
            if (!again || (st[i].err & ~kErrCollision)) continue;  // (other failures stay failures)
            if (h->p2_depth > desc[i].Z + 1) continue;  // not converging: reported as a collision
            redo.push_back(i);
            redo_hint.push_back(std::move(so));
        }
    }
    for (int i = 0; i < nb; ++i) {
        blocks[i].status = st[i].active ? CTWS_BLOCK_WRITTEN : (pl.pass2 ? CTWS_BLOCK_EMPTY_PASS2 : CTWS_BLOCK_EMPTY);
        blocks[i].max_label = st[i].active ? st[i].max_label : 0;
        if (pl.from_seeds) {
            uint64_t mx;
            std::memcpy(&mx, &st[i]._p[2], sizeof(mx));
            blocks[i].max_label = mx;
        }
        // distinct nonzero output ids: the labels, plus the bare offset of unlabelled in-mask
        // voxels (empty block: only that one, watershed.py:310-321); block 0's offset is 0
        const uint32_t bare = (st[i].active ? st[i]._p[0] : 1u) && desc[i].id_offset != 0;
        blocks[i].n_ids = (pl.pass2 || pl.from_seeds) ? -1 : (int32_t)((st[i].active ? st[i].n_cc : 0u) + bare);
        if (!st[i].active) continue;
        if (std::find(redo.begin(), redo.end(), i) != redo.end()) continue;  // filled by the re-run below
        if (in_wide(i)) continue;  // filled by the wide re-run below
        uint32_t err = st[i].err | (regrow_bad ? kErrVerify : 0u);
        if (desc[i].p2hint >= 0 && !soffh.empty() &&
            !std::equal(h->p2_hints[i].begin(), h->p2_hints[i].end(), soffh.begin() + desc[i].sbase))
            err |= kErrCollision;  // the re-runs did not converge
        const int ns = pl.nd_ws == 2 ? desc[i].Z : 1;
        if (pl.pass2) {
            // a slice/block without any seed: watershedsNew seeds from the hmap minima and the
            // result has no new_to_old entry (takeDict, two_pass_watershed.py:173/204) where it
            // is not masked before the lookup (2-D: in-mask voxels; 3-D: every voxel)
            for (int z = 0; z < ns; ++z) {
                const int64_t s0 = desc[i].sbase + z;
                const uint32_t nl = pl.nd_ws == 2 ? ((z + 1 < ns ? sbh[s0 + 1] : st[i].n_seeds) - sbh[s0]) : st[i].n_seeds;
                if (!nl && (pl.nd_ws == 3 || inmask[s0])) err |= kErrTakeDict;
            }
        }
        if (err) {
            blocks[i].status = CTWS_BLOCK_FAILED;
            char msg[256];
            std::snprintf(msg, sizeof msg, "block %lld failed (%s%s%s%s%s%s%s); ", (long long)blocks[i].block_id,
                          (err & kErrHashFull) ? "pass-2 relabel hash table full " : "",
                          (err & kErrCollision) ? "pass-2 2-D wrapped-id merge did not converge " : "",
                          (err & kErrLabelBits) ? "auto-seed labels beyond 2^20 " : "",
                          (err & kErrTakeDict) ? "takeDict: no new_to_old entry, as in the reference " : "",
                          (err & kErrUnsupported) ? "auto-seeded regrow with >= 2^20 seeds " : "",
                          (err & kErrOverflow) ? "seed id >= 2^32 - 1: Overflow detected, as in the reference " : "",
                          (err & kErrVerify) ? "size-filter regrow fixpoint check failed " : "");
            if (err & kErrReserved) h->err += "label 2^64 - 1 is reserved (the seed hash's empty marker) ";
            h->err += msg;
        }
    }
    // per block: an in-mask voxel without a label (its output is the bare id offset), for the
    // host path's widening of the uint32 codes (empty blocks: every in-mask voxel)
    std::vector<uint8_t> bare(nb);
    for (int i = 0; i < nb; ++i) bare[i] = st[i].active ? (st[i]._p[0] != 0) : 1;
    if (!redo.empty()) {
        std::vector<ctws_block> rb;
        std::vector<BlockIO> rio;
        for (int i : redo) {
            rb.push_back(blocks[i]);
            rio.push_back(io[i]);
        }
        auto saved = std::move(h->p2_hints);
        h->p2_hints = std::move(redo_hint);
        ++h->p2_depth;
        const int rr = run_batch(h, cfg, pl, rb.data(), rio.data(), (int)rb.size());
        --h->p2_depth;
        h->p2_hints = std::move(saved);
        if (rr != CTWS_OK) return rr;
        for (size_t k = 0; k < redo.size(); ++k) {
            blocks[redo[k]].status = rb[k].status;
            blocks[redo[k]].max_label = rb[k].max_label;
            blocks[redo[k]].n_ids = rb[k].n_ids;
            if (k < h->last_bare.size()) bare[redo[k]] = h->last_bare[k];  // the re-run's result
        }
        // the device workspace now holds the re-run's blocks only: no block of this call can be
        // read back consistently (ctws_debug_read answers EINVAL)
        h->last_desc.clear();
        add_timing(h, "p2_merge_reruns", (float)redo.size());
    }
    if (!wide.empty()) {
        std::vector<ctws_block> rb;
        std::vector<BlockIO> rio;
        std::vector<std::vector<uint32_t>> rh;
        const bool hints = h->p2_hints.size() == (size_t)nb;
        for (int i : wide) {
            rb.push_back(blocks[i]);
            rio.push_back(io[i]);
            if (hints) rh.push_back(h->p2_hints[i]);
        }
        auto saved = std::move(h->p2_hints);
        h->p2_hints = std::move(rh);
        ++h->wide_rerun;
        const int rr = run_batch(h, cfg, pl, rb.data(), rio.data(), (int)rb.size());
        --h->wide_rerun;
        h->p2_hints = std::move(saved);
        if (rr != CTWS_OK) return rr;
        for (size_t k = 0; k < wide.size(); ++k) {
            blocks[wide[k]].status = rb[k].status;
            blocks[wide[k]].max_label = rb[k].max_label;
            blocks[wide[k]].n_ids = rb[k].n_ids;
            if (k < h->last_bare.size()) bare[wide[k]] = h->last_bare[k];
        }
        h->last_desc.clear();
        add_timing(h, "flood_wide_reruns", (float)wide.size());
    }
    h->last_bare = std::move(bare);
    return CTWS_OK;
}

// Why a block cannot run, or nullptr.  These blocks get CTWS_BLOCK_FAILED with the reason (the
// reference job would raise at that block, or the block is outside what the kernels support)
// while the other blocks of the call run.
const char* block_refusal(const Plan& pl, const ctws_block& b) {
    const int64_t Z = b.outer_shape[0], Y = b.outer_shape[1], X = b.outer_shape[2];
    if (X > kMaxRowX || Y > kMaxColLen || Z > kMaxColLen || Z * Y * X >= (1ll << 31))
        return "outer block too large for the kernels (X <= 10176, Y, Z <= 5088, fewer than 2^31 voxels)";
    // vigra's convolveLine: "kernel longer than line" (the reference raises at this block)
    auto too_short = [&](const double* sg, bool en) -> bool {
        if (!en) return false;
        const int64_t lens[3] = {Z, Y, X};
        for (int a = (pl.nd_ws == 3 ? 0 : 1); a < 3; ++a) {
            if (sg[a] <= 0) continue;
            int r = (int)(3.0 * sg[a] + 0.5);
            if (r == 0) r = 1;
            if (lens[a] < r + 1) return true;
        }
        return false;
    };
    if (!pl.from_seeds && (too_short(pl.sig_seeds, pl.seeds_smooth) || too_short(pl.sig_weights, pl.weights_smooth)))
        return "convolveLine(): kernel longer than line (vigra raises, as the reference job would)";
    return nullptr;
}

int64_t batch_voxels_budget() {
    const char* e = std::getenv("CTWS_BATCH_VOXELS");
    if (e) return std::max<int64_t>(1, std::atoll(e));
    return 512ll << 20;  // ~26 GB of workspace at ~50 B per voxel
}

// ---- host-pointer path: pinned staging, copies overlapped with the compute -----------------
// Batch j uses slot j & 1.  A worker thread packs batch j + 1's inputs into the slot's pinned
// buffer and starts its host-to-device copy on s_in while the calling thread runs batch j on
// the library stream; batch j's outputs go device-to-host on s_out and another worker unpacks
// them into the callers' arrays while batch j + 1 computes.  Events order every reuse of a slot.
// Host copies run on two persistent worker pools of the handle (ctws_host::WorkerPool): one for
// packing, one for widening.  Their sizes (CTWS_PACK_THREADS, CTWS_UNPACK_THREADS) leave a core
// to the calling thread, whose host round trips inside run_batch must not wait for one.
constexpr size_t kCopyChunk = (size_t)4 << 20;  // bytes per pool task

// the copies (dst, src, bytes) in 4 MiB tasks over the pool, streaming stores
void pool_copy(ctws_host::WorkerPool& pool, const std::vector<std::pair<void*, const void*>>& dst_src,
               const std::vector<size_t>& sizes) {
    std::vector<std::pair<size_t, size_t>> tasks;  // (copy index, byte offset)
    for (size_t i = 0; i < sizes.size(); ++i)
        for (size_t o = 0; o < sizes[i]; o += kCopyChunk) tasks.push_back({i, o});
    pool.parallel_for((int64_t)tasks.size(), [&](int64_t t) {
        const size_t i = tasks[t].first, o = tasks[t].second;
        ctws_host::stream_copy((char*)dst_src[i].first + o, (const char*)dst_src[i].second + o,
                               std::min(kCopyChunk, sizes[i] - o));
    });
}

// host <-> device copy in pieces of at most 1 GiB: larger copies are not given to the SDMA
// engines but run as a blit kernel that competes with the compute kernels for the CUs
hipError_t copy_pieces(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    constexpr size_t kPiece = (size_t)1 << 30;
    for (size_t o = 0; o < bytes; o += kPiece) {
        const hipError_t e = hipMemcpyAsync((char*)dst + o, (const char*)src + o, std::min(kPiece, bytes - o), kind, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

int grow_pinned(ctws_handle* h, void*& p, size_t& have, size_t bytes) {
    if (have >= bytes) return CTWS_OK;
    if (p) hipHostFree(p);
    p = nullptr;
    have = 0;
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 256), hipHostMallocDefault) != hipSuccess) {
        h->err = "hipHostMalloc staging failed (" + std::to_string(bytes) + " bytes)";
        return CTWS_ENOMEM;
    }
    have = bytes;
    return CTWS_OK;
}

// uint32 codes of a block's inner region (k_output: the local label) -> the caller's uint64
// output: code + off, except for masked voxels (0).  A zero code is a masked voxel, or -- when
// the block has `bare` voxels (in-mask without a label) -- looked up in the caller's mask.
// Row ranges are the pool's tasks; stores stream past the caches.
void widen_codes(ctws_host::WorkerPool& pool, const ctws_block& b, const uint32_t* codes, uint64_t off, bool bare) {
    const int64_t IY = b.inner_shape[1], IX = b.inner_shape[2];
    const int64_t rows = b.inner_shape[0] * IY;
    const uint8_t* mask = (b.mask && off != 0 && bare) ? b.mask : nullptr;
    const bool masked = b.mask != nullptr && off != 0;
    const int64_t per = std::max<int64_t>(1, (int64_t)(kCopyChunk / 12) / std::max<int64_t>(IX, 1));  // rows per task
    pool.parallel_for((rows + per - 1) / per, [&](int64_t t) {
        const int64_t r0 = t * per, r1 = std::min(rows, r0 + per);
        if (!masked) {
            ctws_host::widen_add(b.output + r0 * IX, codes + r0 * IX, (r1 - r0) * IX, off);
        } else if (!mask) {
            ctws_host::widen_add_nz(b.output + r0 * IX, codes + r0 * IX, (r1 - r0) * IX, off);
        } else {
            for (int64_t r = r0; r < r1; ++r) {
                const uint32_t* c = codes + r * IX;
                uint64_t* o = b.output + r * IX;
                const int64_t z = r / IY, y = r - z * IY;
                const uint8_t* m = mask + ((z + b.inner_begin[0]) * b.outer_shape[1] + (y + b.inner_begin[1])) *
                                              b.outer_shape[2] + b.inner_begin[2];
                for (int64_t x = 0; x < IX; ++x) o[x] = (c[x] || m[x]) ? (uint64_t)c[x] + off : 0ull;
            }
        }
        _mm_sfence();
    });
}

struct HostBatch {
    int k, nb;  // blocks todo[k .. k + nb)
    std::vector<size_t> in_off, in_sz, m_off, i_off, o_off, o_sz;
    size_t in_bytes = 0, out_bytes = 0;
};

int run_blocks_host(ctws_handle* h, const ctws_cfg* cfg, const Plan& pl, ctws_block* blocks,
                    const std::vector<int>& todo) {
    int r;
    // (r02: 8-12 blocks of config 3 per batch, 4.3 Gvoxel/s, against 4.0 at the device budget)
    const int64_t budget = std::min(batch_voxels_budget(), h->host_batch_voxels);
    // batches and their packed layouts (inputs, masks and initial seeds in one buffer)
    std::vector<HostBatch> hb;
    size_t max_in = 0, max_out = 0;
    int64_t rem_vox = 0;
    for (int i : todo) rem_vox += blocks[i].outer_shape[0] * blocks[i].outer_shape[1] * blocks[i].outer_shape[2];
    for (size_t k = 0; k < todo.size();) {
        size_t e = k;
        int64_t vox = 0;
        // ramped batches: the first upload and the last download + widening are not overlapped
        // with compute, so the first two and the last batches are smaller (1/4, 1/2 of the budget)
        int64_t bud = budget;
        if (h->host_ramp) {
            if (hb.size() == 0) bud = budget / 4;
            else if (hb.size() == 1) bud = budget / 2;
            if (rem_vox < 2 * budget) bud = std::min(bud, std::max(budget / 4, rem_vox / 2));
        }
        while (e < todo.size()) {
            const ctws_block& b = blocks[todo[e]];
            const int64_t nv = b.outer_shape[0] * b.outer_shape[1] * b.outer_shape[2];
            if (e > k && (vox + nv > bud || e - k >= 4096 || (h->host_batch_blocks > 0 &&
                                                               (int)(e - k) >= h->host_batch_blocks)))
                break;
            vox += nv;
            ++e;
        }
        rem_vox -= vox;
        HostBatch B;
        B.k = (int)k;
        B.nb = (int)(e - k);
        auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
        for (int i = 0; i < B.nb; ++i) {
            const ctws_block& b = blocks[todo[k + i]];
            const int64_t nv = b.outer_shape[0] * b.outer_shape[1] * b.outer_shape[2];
            const size_t es = b.input_dtype == CTWS_U8 ? 1 : (b.input_dtype == CTWS_U16 ? 2 : (b.input_dtype == CTWS_F32 ? 4 : 8));
            B.in_sz.push_back((size_t)nv * es * (size_t)std::max(1, b.n_channels));
            B.in_off.push_back(B.in_bytes);
            B.in_bytes += al(B.in_sz.back());
            B.m_off.push_back(b.mask ? B.in_bytes : 0);
            if (b.mask) B.in_bytes += al((size_t)nv);
            B.i_off.push_back(b.initial_seeds ? B.in_bytes : 0);
            if (b.initial_seeds) B.in_bytes += al((size_t)nv * 8);
            B.o_sz.push_back((size_t)(b.inner_shape[0] * b.inner_shape[1] * b.inner_shape[2]) * 4);  // uint32 codes
            B.o_off.push_back(B.out_bytes);
            B.out_bytes += al(B.o_sz.back());
        }
        max_in = std::max(max_in, B.in_bytes);
        max_out = std::max(max_out, B.out_bytes);
        hb.push_back(std::move(B));
        k = e;
    }
    if (hb.empty()) return CTWS_OK;
    if (!h->pack_pool) h->pack_pool.reset(new ctws_host::WorkerPool(h->pack_threads));
    if (!h->unpack_pool) h->unpack_pool.reset(new ctws_host::WorkerPool(h->unpack_threads));
    if (!h->s_in) {
        HIPCHK(hipStreamCreateWithFlags(&h->s_in, hipStreamNonBlocking));
        HIPCHK(hipStreamCreateWithFlags(&h->s_out, hipStreamNonBlocking));
        for (auto& sl : h->hslot) {
            HIPCHK(hipEventCreateWithFlags(&sl.ev_h2d, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&sl.ev_comp, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&sl.ev_d2h, hipEventDisableTiming));
            HIPCHK(hipEventCreate(&sl.ev_t0));
            HIPCHK(hipEventCreate(&sl.ev_t1));
        }
    }
    const int nslots = hb.size() > 1 ? 2 : 1;
    for (int s = 0; s < nslots; ++s) {
        auto& sl = h->hslot[s];
        if ((r = grow_pinned(h, sl.pin_in, sl.pin_in_bytes, max_in)) != CTWS_OK) return r;
        if ((r = grow_pinned(h, sl.pin_out, sl.pin_out_bytes, max_out)) != CTWS_OK) return r;
        if ((r = grow(h, sl.d_in, max_in)) != CTWS_OK) return r;
        if ((r = grow(h, sl.d_out, max_out)) != CTWS_OK) return r;
        // a fresh handle's events have never been recorded: mark the slots free
        HIPCHK(hipEventRecord(sl.ev_d2h, h->s_out));
        HIPCHK(hipEventRecord(sl.ev_comp, h->stream));
    }
    // wall times (summed over batches) of the packing, widening and compute phases; the first
    // two run on worker threads, so they are only added to the timings at the end
    double pack_ms = 0.0, unpack_ms = 0.0, compute_ms = 0.0;
    const auto tcall = std::chrono::steady_clock::now();
    auto since = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - tcall).count() * 1e3; };
    // pack batch j's inputs into its slot and start the upload (worker thread)
    // pack batch j's inputs block by block into its slot, each block's upload starting as soon
    // as it is packed (worker thread)
    auto stage_in = [&](int j) -> int {
        const HostBatch& B = hb[j];
        auto& sl = h->hslot[j % nslots];
        // the slot's previous upload is complete (and its batch computed: run_batch returns
        // after its stream drained).  Copies wait on the host, never on another queue's event.
        if (hipEventSynchronize(sl.ev_h2d) != hipSuccess) return CTWS_EHIP;
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < B.nb; ++i) {
            const ctws_block& b = blocks[todo[B.k + i]];
            const int64_t nv = b.outer_shape[0] * b.outer_shape[1] * b.outer_shape[2];
            std::vector<std::pair<void*, const void*>> ds{{(char*)sl.pin_in + B.in_off[i], b.input}};
            std::vector<size_t> sz{B.in_sz[i]};
            if (b.mask) {
                ds.push_back({(char*)sl.pin_in + B.m_off[i], b.mask});
                sz.push_back((size_t)nv);
            }
            if (b.initial_seeds) {
                ds.push_back({(char*)sl.pin_in + B.i_off[i], b.initial_seeds});
                sz.push_back((size_t)nv * 8);
            }
            pool_copy(*h->pack_pool, ds, sz);
            if (h->h2d_mode == 1 && i + 1 < B.nb) continue;  // one copy for the whole batch
            const size_t beg = h->h2d_mode == 1 ? 0 : B.in_off[i];
            const size_t end = i + 1 < B.nb ? B.in_off[i + 1] : B.in_bytes;
            if (i == 0 || h->h2d_mode == 1) {
                if (h->trace) hipEventRecord(sl.ev_t0, h->s_in);
            }
            if (h->h2d_mode == 2) {
                // pull kernel: a few workgroups read the pinned buffer over PCIe
                void* hsrc = nullptr;
                if (hipHostGetDevicePointer(&hsrc, sl.pin_in, 0) != hipSuccess) return CTWS_EHIP;
                k_copy_to_host<<<h->h2d_wgs, 256, 0, h->s_in>>>((const uint4*)((char*)hsrc + beg),
                                                                 (uint4*)((char*)sl.d_in.p + beg), (end - beg + 15) / 16);
                if (hipGetLastError() != hipSuccess) return CTWS_EHIP;
            } else if (copy_pieces((char*)sl.d_in.p + beg, (char*)sl.pin_in + beg, end - beg, hipMemcpyHostToDevice,
                                   h->s_in) != hipSuccess) {
                return CTWS_EHIP;
            }
        }
        if (h->trace) hipEventRecord(sl.ev_t1, h->s_in);
        const double ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
        pack_ms += ms;
        if (h->trace) std::fprintf(stderr, "[ctws] t=%.1f host batch %d: packed+queued in %.1f ms (%zu B)\n", since(), j, ms, B.in_bytes);
        return hipEventRecord(sl.ev_h2d, h->s_in) == hipSuccess ? CTWS_OK : CTWS_EHIP;
    };
    // widen batch j's uint32 codes into the callers' uint64 outputs block by block as their
    // downloads complete (worker thread)
    const uint64_t bvol = (uint64_t)(cfg->block_shape[0] * cfg->block_shape[1] * cfg->block_shape[2]);
    std::vector<std::vector<uint8_t>> bare_of(hb.size());
    auto drain_out = [&](int j, std::vector<ctws_block>* bbp) -> int {
        const HostBatch& B = hb[j];
        auto& sl = h->hslot[j % nslots];
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < B.nb; ++i) {
            const int st = (*bbp)[i].status;
            // nothing written: pass-2 empty (:240-242) or a failed block
            if (st == CTWS_BLOCK_EMPTY_PASS2 || st == CTWS_BLOCK_FAILED) continue;
            if (hipEventSynchronize(sl.ev_blk[i]) != hipSuccess) return CTWS_EHIP;
            const ctws_block& b = blocks[todo[B.k + i]];
            // pass 1: in-mask voxels get + block_id * prod(block_shape); pass 2 / from-seeds
            // outputs are the uint32 values themselves
            const uint64_t off = (pl.pass2 || pl.from_seeds) ? 0ull : (uint64_t)b.block_id * bvol;
            const bool bare = i < (int)bare_of[j].size() ? bare_of[j][i] != 0 : true;
            widen_codes(*h->unpack_pool, b, (const uint32_t*)((char*)sl.pin_out + B.o_off[i]), off, bare);
        }
        const double ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3;
        unpack_ms += ms;
        if (h->trace) std::fprintf(stderr, "[ctws] t=%.1f host batch %d: widened in %.1f ms (%zu B)\n", since(), j, ms, B.out_bytes);
        return CTWS_OK;
    };
    for (auto& sl : h->hslot) HIPCHK(hipEventRecord(sl.ev_h2d, h->s_in));
    int rin = stage_in(0);
    if (rin != CTWS_OK) return rin;
    std::vector<std::vector<ctws_block>> bbs(hb.size());
    std::thread t_in, t_out;
    int r_in = CTWS_OK, r_out = CTWS_OK;
    auto join_all = [&]() {
        if (t_in.joinable()) t_in.join();
        if (t_out.joinable()) t_out.join();
    };
    for (size_t j = 0; j < hb.size(); ++j) {
        const HostBatch& B = hb[j];
        auto& sl = h->hslot[j % nslots];
        if (j + 1 < hb.size()) t_in = std::thread([&, j]() { r_in = stage_in((int)j + 1); });
        std::vector<ctws_block>& bb = bbs[j];
        bb.resize(B.nb);
        std::vector<BlockIO> io(B.nb);
        for (int i = 0; i < B.nb; ++i) {
            bb[i] = blocks[todo[B.k + i]];
            const ctws_block& b = bb[i];
            io[i].in = (char*)sl.d_in.p + B.in_off[i];
            io[i].mask = b.mask ? (const uint8_t*)((char*)sl.d_in.p + B.m_off[i]) : nullptr;
            io[i].init = b.initial_seeds ? (const uint64_t*)((char*)sl.d_in.p + B.i_off[i]) : nullptr;
            io[i].out = nullptr;
            io[i].out32 = (uint32_t*)((char*)sl.d_out.p + B.o_off[i]);
        }
        // inputs uploaded; the slot's previous outputs downloaded
        if (hipEventSynchronize(sl.ev_h2d) != hipSuccess || hipEventSynchronize(sl.ev_d2h) != hipSuccess) {
            join_all();
            return CTWS_EHIP;
        }
        if (h->trace) {
            float up = 0.f;
            hipEventElapsedTime(&up, sl.ev_t0, sl.ev_t1);
            std::fprintf(stderr, "[ctws] t=%.1f host batch %zu: inputs on the device (first copy -> last: %.1f ms)\n",
                         since(), j, up);
        }
        const auto tb = std::chrono::steady_clock::now();
        if ((r = run_batch(h, cfg, pl, bb.data(), io.data(), B.nb)) != CTWS_OK) {
            join_all();
            return r;
        }
        {
            const double ms = std::chrono::duration<double>(std::chrono::steady_clock::now() - tb).count() * 1e3;
            compute_ms += ms;
            if (h->trace) std::fprintf(stderr, "[ctws] t=%.1f host batch %zu (%d blocks): computed in %.1f ms\n", since(), j, B.nb, ms);
        }
        HIPCHK(hipEventRecord(sl.ev_comp, h->stream));
        bare_of[j] = h->last_bare;
        // the slot's pinned outputs are free once the drain of batch j - 2 finished
        if (t_out.joinable()) t_out.join();
        if (r_out != CTWS_OK) {
            join_all();
            return r_out;
        }
        // download block by block, an event after each
        while ((int)sl.ev_blk.size() < B.nb) {
            hipEvent_t e;
            HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            sl.ev_blk.push_back(e);
        }
        hipError_t ce = hipSuccess;
        void* hdst = nullptr;
        if (h->d2h_wgs > 0) ce = hipHostGetDevicePointer(&hdst, sl.pin_out, 0);
        for (int i = 0; i < B.nb && ce == hipSuccess; ++i) {
            const size_t o = B.o_off[i], nbytes = (B.o_sz[i] + 15) & ~(size_t)15;
            if (h->d2h_wgs > 0) {
                k_copy_to_host<<<h->d2h_wgs, 256, 0, h->s_out>>>((const uint4*)((char*)sl.d_out.p + o),
                                                                  (uint4*)((char*)hdst + o), nbytes / 16);
                ce = hipGetLastError();
            } else {
                ce = copy_pieces((char*)sl.pin_out + o, (char*)sl.d_out.p + o, B.o_sz[i], hipMemcpyDeviceToHost,
                                 h->s_out);
            }
            if (ce == hipSuccess) ce = hipEventRecord(sl.ev_blk[i], h->s_out);
        }
        if (ce != hipSuccess ||
            hipEventRecord(sl.ev_d2h, h->s_out) != hipSuccess) {
            join_all();
            return CTWS_EHIP;
        }
        t_out = std::thread([&, j]() { r_out = drain_out((int)j, &bbs[j]); });
        if (t_in.joinable()) t_in.join();
        if (r_in != CTWS_OK) {
            join_all();
            return r_in;
        }
        for (int i = 0; i < B.nb; ++i) {
            blocks[todo[B.k + i]].status = bb[i].status;
            blocks[todo[B.k + i]].n_ids = bb[i].n_ids;
            blocks[todo[B.k + i]].max_label = bb[i].max_label;
        }
    }
    join_all();
    add_timing(h, "host_pack_ms", (float)pack_ms);
    add_timing(h, "host_unpack_ms", (float)unpack_ms);
    add_timing(h, "host_compute_ms", (float)compute_ms);
    add_timing(h, "host_batches", (float)hb.size());
    return r_out;
}

int run_blocks(ctws_handle* h, const ctws_cfg* cfg_in, ctws_block* blocks, int n, bool device_ptrs,
               bool from_seeds = false, bool sf_fill = false) {
    if (!h || !cfg_in || (!blocks && n > 0) || n < 0) return CTWS_EINVAL;
    h->err.clear();
    h->timings.clear();
    HIPCHK(hipSetDevice(h->device));
    ctws_cfg fcfg = *cfg_in;
    if (from_seeds) {
        // watershed_from_seeds.py: 3-D watershedsNew on the normalized input, no dt / smoothing
        fcfg.apply_ws_2d = fcfg.apply_dt_2d = 0;
        fcfg.has_pixel_pitch = 0;
        fcfg.sigma_seeds_is_list = fcfg.sigma_weights_is_list = 0;
        fcfg.sigma_seeds[0] = fcfg.sigma_weights[0] = 0.0;
        fcfg.invert_inputs = 0;
        fcfg.pass_id = 0;
        for (int i = 0; i < n; ++i) {
            ctws_block& b = blocks[i];
            for (int k = 0; k < 3; ++k) {
                if (b.inner_begin[k] != 0 || b.inner_shape[k] != b.outer_shape[k]) {
                    h->err = "WatershedFromSeeds blocks have no halo: inner block == block";
                    return CTWS_EINVAL;
                }
            }
            if (!b.initial_seeds) {
                h->err = "WatershedFromSeeds needs the seeds (ds_seeds[bb]) of every block";
                return CTWS_EINVAL;
            }
        }
    }
    const ctws_cfg* cfg = &fcfg;
    Plan pl;
    int r = make_plan(h, cfg, pl);
    if (r != CTWS_OK) return r;
    pl.from_seeds = from_seeds ? 1 : 0;
    pl.sf_fill = sf_fill ? 1 : 0;
    // blocks whose inner mask is empty are skipped entirely (watershed.py:290-297); the
    // host-pointer path checks this on the host, the device path on the caller's side
    std::vector<int> todo;
    for (int i = 0; i < n; ++i) {
        ctws_block& b = blocks[i];
        b.status = CTWS_BLOCK_WRITTEN;
        b.n_ids = 0;
        b.max_label = 0;
        if (const char* why = block_refusal(pl, b)) {
            b.status = CTWS_BLOCK_FAILED;
            h->err += "block " + std::to_string((long long)b.block_id) + " failed (" + why + "); ";
            continue;
        }
        if (!device_ptrs && b.mask) {
            const int64_t* sh = b.outer_shape;
            bool any = false;
            for (int64_t z = 0; z < b.inner_shape[0] && !any; ++z)
                for (int64_t y = 0; y < b.inner_shape[1] && !any; ++y) {
                    const uint8_t* row = b.mask + ((z + b.inner_begin[0]) * sh[1] + (y + b.inner_begin[1])) * sh[2] +
                                         b.inner_begin[2];
                    for (int64_t x = 0; x < b.inner_shape[2]; ++x)
                        if (row[x]) {
                            any = true;
                            break;
                        }
                }
            if (!any) {
                b.status = CTWS_BLOCK_SKIPPED_MASK;
                continue;
            }
        }
        todo.push_back(i);
    }
    if (!device_ptrs) return run_blocks_host(h, cfg, pl, blocks, todo);
    const int64_t budget = batch_voxels_budget();
    size_t k = 0;
    while (k < todo.size()) {
        // batch [k, e)
        size_t e = k;
        int64_t vox = 0;
        while (e < todo.size()) {
            const ctws_block& b = blocks[todo[e]];
            const int64_t nv = b.outer_shape[0] * b.outer_shape[1] * b.outer_shape[2];
            if (e > k && (vox + nv > budget || e - k >= 4096)) break;  // <= 4096 blocks (worklist entries)
            vox += nv;
            ++e;
        }
        const int nb = (int)(e - k);
        std::vector<ctws_block> bb(nb);
        std::vector<BlockIO> io(nb);
        for (int i = 0; i < nb; ++i) bb[i] = blocks[todo[k + i]];
        if (device_ptrs) {
            for (int i = 0; i < nb; ++i)
                io[i] = {bb[i].input, bb[i].mask, bb[i].initial_seeds, bb[i].output};
            if ((r = run_batch(h, cfg, pl, bb.data(), io.data(), nb)) != CTWS_OK) return r;
        } else {
            if ((r = run_batch(h, cfg, pl, bb.data(), io.data(), nb)) != CTWS_OK) return r;
        }
        for (int i = 0; i < nb; ++i) {
            blocks[todo[k + i]].status = bb[i].status;
            blocks[todo[k + i]].n_ids = bb[i].n_ids;
            blocks[todo[k + i]].max_label = bb[i].max_label;
        }
        k = e;
    }
    return CTWS_OK;
}

}  // namespace

// =========================================================================================
extern "C" {

int ctws_abi_version(void) { return CTWS_ABI_VERSION; }

int ctws_open(int device, ctws_handle** out) {
    if (!out) return CTWS_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return CTWS_EHIP;
    if (device < 0 || device >= n) return CTWS_EINVAL;
    ctws_handle* h = new ctws_handle();
    h->device = device;
    if (const char* t = std::getenv("CTWS_TRACE")) h->trace = std::atoi(t);
    if (const char* t = std::getenv("CTWS_NO_DESCENT")) h->no_descent = std::atoi(t);
    if (const char* t = std::getenv("CTWS_SEED_TILECC")) h->seed_tilecc = std::atoi(t);
    if (const char* t = std::getenv("CTWS_SEED_DENSE")) h->seed_dense = std::atoi(t);
    if (const char* t = std::getenv("CTWS_NO_FALLBACK")) h->no_fallback = std::atoi(t);
    if (const char* t = std::getenv("CTWS_FORCE_WIDE")) h->force_wide = std::atoi(t);
    if (const char* t = std::getenv("CTWS_SF_SPARSE")) h->sf_sparse = std::atoi(t);
    if (const char* t = std::getenv("CTWS_FUSE_HIST")) h->fuse_hist = std::atoi(t);
    if (const char* t = std::getenv("CTWS_VERIFY")) h->verify = std::atoi(t);
    if (const char* t = std::getenv("CTWS_PREP_LDS")) h->prep_lds = std::atoi(t);
    if (const char* t = std::getenv("CTWS_EDT_BITS")) h->edt_bits = std::atoi(t);
    if (const char* t = std::getenv("CTWS_FRONTIER_ITERS"))
        h->frontier_max_iters = std::max(0, std::min(kFrontierMaxItersCap, std::atoi(t)));
    if (const char* t = std::getenv("CTWS_GAUSS_YX")) h->gauss_yx = std::atoi(t);
    if (const char* t = std::getenv("CTWS_HOST_BATCH_VOXELS")) h->host_batch_voxels = std::max<int64_t>(1, std::atoll(t));
    if (const char* t = std::getenv("CTWS_HOST_RAMP")) h->host_ramp = std::atoi(t);
    if (const char* t = std::getenv("CTWS_PLATEAU_FILL")) h->plateau_fill = std::atoi(t);
    if (const char* t = std::getenv("CTWS_OUTPUT_TILE")) h->output_tile = std::atoi(t);
    if (const char* t = std::getenv("CTWS_H2D_MODE")) h->h2d_mode = std::atoi(t);
    if (const char* t = std::getenv("CTWS_H2D_WGS")) h->h2d_wgs = std::max(1, std::atoi(t));
    if (const char* t = std::getenv("CTWS_HOST_BATCH_BLOCKS")) h->host_batch_blocks = std::max(0, std::atoi(t));
    if (const char* t = std::getenv("CTWS_PACK_THREADS")) h->pack_threads = std::max(1, std::atoi(t));
    if (const char* t = std::getenv("CTWS_UNPACK_THREADS")) h->unpack_threads = std::max(1, std::atoi(t));
    if (const char* t = std::getenv("CTWS_D2H_WGS")) h->d2h_wgs = std::max(0, std::atoi(t));
    if (const char* t = std::getenv("CTWS_WORDS_PER_WAVE")) h->words_per_wave = std::max(1, std::atoi(t));
    if (const char* t = std::getenv("CTWS_GAUSS_W")) {
        const int v = std::atoi(t);
        h->gauss_w = (v == 8 || v == 16 || v == 32) ? v : 0;
    }
    if (const char* t = std::getenv("CTWS_EDT_W")) {
        const int v = std::atoi(t);
        h->edt_w = (v == 8 || v == 16 || v == 32 || v == 64) ? v : 0;
    }
    if (const char* t = std::getenv("CTWS_EDT_WZ")) {
        const int v = std::atoi(t);
        h->edt_wz = (v == 8 || v == 16 || v == 32 || v == 64) ? v : 0;
    }
    auto parse_chunk = [](const char* t, int* c, bool three_d) {
        int a = 0, b = 0, d = 0;
        if (std::sscanf(t, "%dx%dx%d", &a, &b, &d) == 3 && frontier_chunk_ok(three_d ? 3 : 2, a, b, d)) {
            c[0] = a;
            c[1] = b;
            c[2] = d;
        }
    };
    if (const char* t = std::getenv("CTWS_FRONTIER_CHUNK2D")) parse_chunk(t, h->fchunk2, false);
    if (const char* t = std::getenv("CTWS_FRONTIER_CHUNK3D")) {
        parse_chunk(t, h->fchunk3, true);
        h->fchunk3_env = 1;
    }
    if (const char* t = std::getenv("CTWS_FRONTIER_GRID")) h->frontier_grid = std::max(1, std::atoi(t));
    if (const char* t = std::getenv("CTWS_FRONTIER_REPS")) h->frontier_reps = std::max(1, std::atoi(t));
    if (const char* t = std::getenv("CTWS_FRONTIER_DIR")) h->frontier_dir = std::atoi(t) ? 1 : 0;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void**)&h->h_counter, kCounterBytes, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&h->h_taps, 6 * kTapSlot * sizeof(double), hipHostMallocDefault) != hipSuccess) {
        delete h;
        return CTWS_EHIP;
    }
    *out = h;
    return CTWS_OK;
}

void ctws_close(ctws_handle* h) {
    if (!h) return;
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    Workspace& w = h->ws;
    void* ptrs[] = {w.fin, w.dt, w.A, w.Bf, w.sm, w.hm, w.cls, w.P, w.PF, w.lab, w.key, w.W, w.Wp, w.csum,
                    w.smin, w.smax, w.sb, w.slmax, w.soff, w.surv, w.act0, w.act1, w.lines0, w.lines1, w.desc, w.stat, w.counter,
                    w.taps, w.hkey, w.hpos, w.p2err, w.front0, w.front1, w.fopen, w.fflags, w.fchunk0, w.fchunk1, w.wl0, w.wl1, w.qgen, w.wlcnt,
                    w.fstat, w.sfacc, h->st_in.p, h->st_mask.p, h->st_init.p, h->st_out.p, h->rl_lab.p, h->rl_bits.p,
                    h->rl_cnt.p, h->rl_offs.p, h->rl_out.p, h->rl_keys.p, h->rl_vals.p, h->rl_red.p,
                    h->edt_fh.p, h->edt_scratch.p, h->p2_hint_dev.p, h->rl_sorted.p, h->rl_uniq.p, h->rl_counts.p, h->rl_tmp.p,
                    h->fs_vals.p, h->fs_sorted.p, h->fs_off.p, h->fs_tmp.p, h->sf_ids.p, h->sf_bits.p, h->sf_desc.p,
                    h->sf_stat.p, h->sf_seeds.p, h->sf_lab.p, h->sf_hm.p, h->sf_out.p, h->ev_ka.p, h->ev_ca.p, h->ev_kb.p,
                    h->ev_cb.p, h->ev_kp.p, h->ev_cp.p, h->ev_state.p, h->ev_out.p, h->ev_stage.p,
                    w.fplat, w.plev, w.fseed, h->tc_P.p, h->tc_bits.p, h->tc_cnt.p, h->tc_offs.p, h->tc_woff.p,
                    h->tc_red.p, h->tc_in.p, h->tc_mask.p, h->tc_out.p, h->tc_raw.p, h->tc_tmp.p, h->tc_taps.p,
                    h->rg_lab.p, h->rg_tab.p, h->rg_nodes.p, h->rg_pairs.p, h->rg_w.p, h->rg_keys.p, h->rg_skeys.p, h->rg_sw.p,
                    h->rg_sum.p, h->rg_out.p, h->rg_tmp.p, h->rg_red.p, h->ef_lab.p, h->ef_data.p, h->ef_nodes.p,
                    h->ef_edges.p, h->ef_out.p, h->ef_ekeys.p, h->ef_keys.p, h->ef_skeys.p, h->ef_tmp.p, h->ef_red.p,
                    h->ov_lab.p, h->ov_rows.p, h->mo_rows.p, h->mo_acc.p, h->rf_data.p, h->rf_rows.p,
                    h->rf_cnt.p, h->rf_off.p, h->rf_sums.p, h->rf_ctab.p, h->ds_in.p, h->ds_out.p,
                    h->ds_flag.p, h->rc_lab.p, h->rc_objs.p, h->rc_list.p, h->rc_keys.p, h->rc_cent.p,
                    h->rc_found.p, h->rc_a.p, h->rc_b.p, h->if_in.p, h->if_out.p, h->if_a.p, h->if_b.p,
                    h->if_taps.p, h->if_mm.p, h->lf_edges.p, h->lf_lab.p, h->lf_out.p, h->lf_deg.p, h->lf_row.p,
                    h->lf_adj.p, h->lf_src.p, h->lf_queue.p, h->lf_bits.p, h->lf_keys.p, h->lf_skeys.p, h->lf_tmp.p,
                    h->lf_red.p, h->gp_edges.p, h->gp_w.p, h->gp_in.p, h->gp_out.p, h->gp_parent.p, h->gp_next.p,
                    h->gp_best.p, h->gp_num.p, h->gp_su.p, h->gp_sv.p, h->gp_keys.p, h->gp_skeys.p, h->gp_idx.p,
                    h->gp_sidx.p, h->gp_tmp.p, h->gp_red.p};
    for (void* p : ptrs)
        if (p) hipFree(p);
    for (auto e : h->events) hipEventDestroy(e);
    for (auto e : h->fev)
        if (e) hipEventDestroy(e);
    if (h->h_counter) hipHostFree(h->h_counter);
    if (h->h_taps) hipHostFree(h->h_taps);
    for (auto& sl : h->hslot) {
        if (sl.pin_in) hipHostFree(sl.pin_in);
        if (sl.pin_out) hipHostFree(sl.pin_out);
        if (sl.d_in.p) hipFree(sl.d_in.p);
        if (sl.d_out.p) hipFree(sl.d_out.p);
        for (hipEvent_t e : {sl.ev_h2d, sl.ev_comp, sl.ev_d2h, sl.ev_t0, sl.ev_t1})
            if (e) hipEventDestroy(e);
        for (hipEvent_t e : sl.ev_blk) hipEventDestroy(e);
    }
    if (h->s_in) hipStreamDestroy(h->s_in);
    if (h->s_out) hipStreamDestroy(h->s_out);
    hipStreamDestroy(h->stream);
    delete h;
}

const char* ctws_last_error(const ctws_handle* h) { return h ? h->err.c_str() : "null handle"; }

int ctws_ws_blocks(ctws_handle* h, const ctws_cfg* cfg, ctws_block* blocks, int n_blocks) {
    return run_blocks(h, cfg, blocks, n_blocks, false);
}

int ctws_ws_blocks_device(ctws_handle* h, const ctws_cfg* cfg, ctws_block* blocks, int n_blocks) {
    return run_blocks(h, cfg, blocks, n_blocks, true);
}

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

int ctws_ws_from_seeds(ctws_handle* h, const ctws_cfg* cfg, ctws_block* blocks, int n_blocks) {
    return run_blocks(h, cfg, blocks, n_blocks, false, true);
}

int ctws_ws_from_seeds_device(ctws_handle* h, const ctws_cfg* cfg, ctws_block* blocks, int n_blocks) {
    return run_blocks(h, cfg, blocks, n_blocks, true, true);
}

// ---- SizeFilterWorkflow: BackgroundSizeFilter / FillingSizeFilter blocks ---------------------
namespace {

// a discard set whose id range is at most this wide is kept as a bitmap too (32 MiB)
constexpr uint64_t kSfBitmapRange = 1ull << 28;

size_t sf_al(size_t v) { return (v + 255) & ~(size_t)255; }

// One batch (blocks[idx[..]]): membership of every voxel's id in the resident discard set, the
// per-block facts, and from them what apply_block does (background_size_filter.py:110-130,
// filling_size_filter.py:112-136).  The blocks that need the fill run on the from_seeds plan
// (run_blocks with sf_fill) with the zeroed labels as seeds.
int sf_batch(ctws_handle* h, ctws_block* blocks, const std::vector<int>& idx, int fill, bool dev, std::string& errs,
             std::vector<std::pair<const char*, float>>& timings) {
    const int nb = (int)idx.size();
    int r;
    std::vector<int64_t> N(nb), off(nb);
    int64_t T = 0, maxN = 0;
    for (int i = 0; i < nb; ++i) {
        const ctws_block& b = blocks[idx[i]];
        N[i] = b.outer_shape[0] * b.outer_shape[1] * b.outer_shape[2];
        off[i] = T;
        T += N[i];
        maxN = std::max(maxN, N[i]);
    }
    if ((r = grow(h, h->sf_seeds, sizeof(uint64_t) * (size_t)T)) != CTWS_OK) return r;
    if ((r = grow(h, h->sf_desc, sizeof(SfBlock) * (size_t)nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->sf_stat, sizeof(BlockStat) * (size_t)nb)) != CTWS_OK) return r;
    if (!dev && (r = grow(h, h->sf_lab, sizeof(uint64_t) * (size_t)T)) != CTWS_OK) return r;
    uint64_t* seeds = (uint64_t*)h->sf_seeds.p;
    std::vector<SfBlock> sd(nb);
    for (int i = 0; i < nb; ++i) {
        const ctws_block& b = blocks[idx[i]];
        if (dev) {
            sd[i].lab = b.initial_seeds;
        } else {
            uint64_t* l = (uint64_t*)h->sf_lab.p + off[i];
            HIPCHK(copy_pieces(l, b.initial_seeds, sizeof(uint64_t) * (size_t)N[i], hipMemcpyHostToDevice, h->stream));
            sd[i].lab = l;
        }
        sd[i].seeds = seeds + off[i];
        sd[i].N = N[i];
    }
    HIPCHK(hipMemcpyAsync(h->sf_desc.p, sd.data(), sizeof(SfBlock) * nb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->sf_stat.p, 0, sizeof(BlockStat) * nb, h->stream));
    SfDiscard d;
    d.ids = (const uint64_t*)h->sf_ids.p;
    d.n = h->sf_n;
    d.bits = h->sf_has_bits ? (const uint64_t*)h->sf_bits.p : nullptr;
    d.lo = h->sf_n ? h->sf_lo : 1ull;
    d.hi = h->sf_n ? h->sf_hi : 0ull;
    record(h, 0);
    const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>((maxN + 255) / 256, 4096)), nb);
    k_sf_member<<<g, 256, 0, h->stream>>>((const SfBlock*)h->sf_desc.p, (BlockStat*)h->sf_stat.p, d);
    LAUNCHCHK();
    record(h, 1);
    std::vector<BlockStat> st(nb);
    HIPCHK(hipMemcpyAsync(st.data(), h->sf_stat.p, sizeof(BlockStat) * nb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    {
        float ms = 0.f;
        hipEventElapsedTime(&ms, h->events[0], h->events[1]);
        timings.push_back({"sf_member", ms});
    }
    // the fill's blocks: height maps and outputs on the device
    std::vector<int> fi;
    size_t hm_bytes = 0, out_elems = 0;
    std::vector<size_t> hm_off(nb, 0), out_off(nb, 0);
    for (int i = 0; i < nb; ++i) {
        ctws_block& b = blocks[idx[i]];
        b.n_ids = -1;
        std::memcpy(&b.max_label, &st[i]._p[2], sizeof(uint64_t));
        if (!st[i].active) {
            b.status = CTWS_BLOCK_ZERO;  // every label 0: nothing written (:117-120)
            b.max_label = 0;
        } else if (!st[i].fg) {
            b.status = CTWS_BLOCK_COPIED;  // no voxel carries a discard id: the labels (:123-128)
            if (b.output != b.initial_seeds) {
                if (dev) HIPCHK(copy_pieces(b.output, b.initial_seeds, sizeof(uint64_t) * (size_t)N[i], hipMemcpyDeviceToDevice, h->stream));
                else std::memcpy(b.output, b.initial_seeds, sizeof(uint64_t) * (size_t)N[i]);
            }
        } else if (!fill) {
            b.status = CTWS_BLOCK_WRITTEN;
            HIPCHK(copy_pieces(b.output, seeds + off[i], sizeof(uint64_t) * (size_t)N[i],
                               dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
        } else {
            hm_off[i] = hm_bytes;
            hm_bytes += sf_al((size_t)N[i] * (b.input_dtype == CTWS_U8 ? 1 : b.input_dtype == CTWS_U16 ? 2 : 4));
            out_off[i] = out_elems;
            out_elems += (size_t)N[i];
            fi.push_back(i);
        }
    }
    if (!fi.empty()) {
        if (!dev) {
            if ((r = grow(h, h->sf_hm, hm_bytes)) != CTWS_OK) return r;
            if ((r = grow(h, h->sf_out, sizeof(uint64_t) * out_elems)) != CTWS_OK) return r;
        }
        std::vector<ctws_block> fb;
        for (int i : fi) {
            ctws_block b = blocks[idx[i]];
            if (!dev) {
                const size_t es = b.input_dtype == CTWS_U8 ? 1 : b.input_dtype == CTWS_U16 ? 2 : 4;
                HIPCHK(copy_pieces((char*)h->sf_hm.p + hm_off[i], b.input, (size_t)N[i] * es, hipMemcpyHostToDevice,
                                   h->stream));
                b.input = (char*)h->sf_hm.p + hm_off[i];
                b.output = (uint64_t*)h->sf_out.p + out_off[i];
            }
            b.initial_seeds = seeds + off[i];
            b.mask = nullptr;
            fb.push_back(b);
        }
        HIPCHK(hipStreamSynchronize(h->stream));
        ctws_cfg cfg;
        std::memset(&cfg, 0, sizeof(cfg));
        cfg.channel_end = -1;
        cfg.block_shape[0] = cfg.block_shape[1] = cfg.block_shape[2] = 1;
        r = run_blocks(h, &cfg, fb.data(), (int)fb.size(), true, true, true);
        errs += h->err;
        for (auto& t : h->timings) timings.push_back(t);
        if (r != CTWS_OK) return r;
        for (size_t k = 0; k < fi.size(); ++k) {
            ctws_block& b = blocks[idx[fi[k]]];
            b.status = fb[k].status;
            b.max_label = fb[k].max_label;
            if (!dev && b.status == CTWS_BLOCK_WRITTEN)
                HIPCHK(copy_pieces(b.output, fb[k].output, sizeof(uint64_t) * (size_t)N[fi[k]], hipMemcpyDeviceToHost,
                                   h->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTWS_OK;
}

int sf_blocks(ctws_handle* h, ctws_block* blocks, int n, int fill, bool dev) {
    if (!h || (!blocks && n > 0) || n < 0) return CTWS_EINVAL;
    h->err.clear();
    h->timings.clear();
    HIPCHK(hipSetDevice(h->device));
    std::string errs;
    std::vector<int> todo;
    for (int i = 0; i < n; ++i) {
        ctws_block& b = blocks[i];
        b.status = CTWS_BLOCK_WRITTEN;
        b.n_ids = -1;
        b.max_label = 0;
        if (!b.initial_seeds || !b.output || (fill && !b.input)) {
            h->err = "size filter blocks need labels (initial_seeds), an output and, for the fill, a height map (input)";
            return CTWS_EINVAL;
        }
        for (int k = 0; k < 3; ++k)
            if (b.outer_shape[k] <= 0 || b.inner_begin[k] != 0 || b.inner_shape[k] != b.outer_shape[k]) {
                h->err = "size filter blocks have no halo: inner block == block";
                return CTWS_EINVAL;
            }
        if (fill && (b.n_channels != 0 || (b.input_dtype != CTWS_U8 && b.input_dtype != CTWS_U16 && b.input_dtype != CTWS_F32))) {
            b.status = CTWS_BLOCK_FAILED;
            errs += "block " + std::to_string((long long)b.block_id) + " failed (the filling size filter takes a 3-D " +
                    "uint8, uint16 or float32 height map: the flood runs on its float32 values exactly, which a " +
                    (b.n_channels != 0 ? "multi-channel" : "float64 or other") + " map does not give); ";
            continue;
        }
        todo.push_back(i);
    }
    std::vector<std::pair<const char*, float>> timings;
    const int64_t budget = dev ? batch_voxels_budget() : std::min(batch_voxels_budget(), h->host_batch_voxels);
    int r = CTWS_OK;
    for (size_t k = 0; k < todo.size() && r == CTWS_OK;) {
        std::vector<int> idx;
        int64_t vox = 0;
        while (k < todo.size()) {
            const ctws_block& b = blocks[todo[k]];
            const int64_t nv = b.outer_shape[0] * b.outer_shape[1] * b.outer_shape[2];
            if (!idx.empty() && (vox + nv > budget || idx.size() >= 4096)) break;
            vox += nv;
            idx.push_back(todo[k++]);
        }
        r = sf_batch(h, blocks, idx, fill, dev, errs, timings);
    }
    const std::string last = h->err;
    h->err = errs;
    if (r != CTWS_OK && errs.find(last) == std::string::npos) h->err += last;
    h->timings.clear();
    for (auto& t : timings) {
        if (std::strcmp(t.first, "prep_kernel") == 0) set_timing(h, t.first, t.second);
        else add_timing(h, t.first, t.second);
    }
    return r;
}

}  // namespace

int ctws_set_discard_u64(ctws_handle* h, const uint64_t* ids, int64_t n) {
    if (!h || n < 0 || (n > 0 && !ids)) return CTWS_EINVAL;
    h->err.clear();
    HIPCHK(hipSetDevice(h->device));
    for (int64_t i = 1; i < n; ++i)
        if (ids[i] <= ids[i - 1]) {
            h->err = "discard ids must be strictly ascending";
            return CTWS_EINVAL;
        }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->sf_n = 0;
    h->sf_has_bits = false;
    if (n == 0) return CTWS_OK;
    int r;
    if ((r = grow(h, h->sf_ids, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
    HIPCHK(hipMemcpy(h->sf_ids.p, ids, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice));
    const uint64_t lo = ids[0], hi = ids[n - 1];
    if (hi - lo < kSfBitmapRange) {
        std::vector<uint64_t> bits((size_t)((hi - lo) >> 6) + 1, 0ull);
        for (int64_t i = 0; i < n; ++i) bits[(ids[i] - lo) >> 6] |= 1ull << ((ids[i] - lo) & 63);
        if ((r = grow(h, h->sf_bits, sizeof(uint64_t) * bits.size())) != CTWS_OK) return r;
        HIPCHK(hipMemcpy(h->sf_bits.p, bits.data(), sizeof(uint64_t) * bits.size(), hipMemcpyHostToDevice));
        h->sf_has_bits = true;
    }
    h->sf_lo = lo;
    h->sf_hi = hi;
    h->sf_n = n;
    return CTWS_OK;
}

int ctws_size_filter_blocks(ctws_handle* h, ctws_block* blocks, int n_blocks, int fill) {
    return sf_blocks(h, blocks, n_blocks, fill ? 1 : 0, false);
}

int ctws_size_filter_blocks_device(ctws_handle* h, ctws_block* blocks, int n_blocks, int fill) {
    return sf_blocks(h, blocks, n_blocks, fill ? 1 : 0, true);
}

int ctws_last_timings(const ctws_handle* h, const char** names, float* ms, int max_entries) {
    if (!h) return 0;
    const int n = (int)std::min<size_t>(h->timings.size(), (size_t)std::max(0, max_entries));
    for (int i = 0; i < n; ++i) {
        if (names) names[i] = h->timings[i].first;
        if (ms) ms[i] = h->timings[i].second;
    }
    return (int)h->timings.size();
}

int ctws_debug_set_stop(ctws_handle* h, int stage) {
    if (!h || stage < 0 || stage > 3) return CTWS_EINVAL;
    h->stop_after = stage;
    return CTWS_OK;
}

int ctws_debug_sqrt_int(ctws_handle* h, uint32_t n0, uint32_t count, float* dst) {
    if (!h || !dst || count == 0u || (uint64_t)n0 + count > (1ull << 24)) return CTWS_EINVAL;
    HIPCHK(hipSetDevice(h->device));
    float* d = nullptr;
    HIPCHK(hipMalloc(&d, sizeof(float) * (size_t)count));
    k_sqrt_int_check<<<(count + 255u) / 256u, 256, 0, h->stream>>>(n0, count, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(dst, d, sizeof(float) * (size_t)count, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    hipFree(d);
    if (e != hipSuccess) {
        h->err = hipGetErrorString(e);
        return CTWS_EHIP;
    }
    return CTWS_OK;
}

int ctws_debug_read(ctws_handle* h, const char* array, int block, void* dst, int64_t nbytes) {
    if (!h || !array || !dst || block < 0 || block >= (int)h->last_desc.size()) return CTWS_EINVAL;
    const BlockDesc& d = h->last_desc[block];
    const Workspace& w = h->ws;
    const std::string a(array);
    const void* src = nullptr;
    size_t es = 4;
    if (a == "fin") src = w.fin;
    else if (a == "dt") src = w.dt;
    else if (a == "seedmap") src = w.sm;
    else if (a == "hmap") src = w.hm;
    else if (a == "labels") src = w.lab;
    else if (a == "cls") { src = w.cls; es = 1; }
    else return CTWS_EINVAL;
    if (nbytes != (int64_t)(d.N * es)) {
        h->err = "ctws_debug_read: nbytes must be N * itemsize";
        return CTWS_EINVAL;
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(dst, (const char*)src + d.base * es, (size_t)nbytes, hipMemcpyDeviceToHost));
    return CTWS_OK;
}

}  // extern "C"

namespace {
// np.unique(labels[, return_counts]) by radix sort + run-length encoding (k_relabel.hip): any
// value range.  dl: device labels; out / counts: caller buffers (device or host), cap entries.
int unique_sorted(ctws_handle* h, const uint64_t* dl, int64_t n, int on_device, uint64_t* out, uint64_t* counts,
                  int64_t cap, int64_t* n_unique) {
    if (n >= (1ll << 31)) {
        h->err = "unique: more than 2^31 - 1 labels in one call";
        return CTWS_EUNSUPPORTED;
    }
    int r;
    size_t tb_sort = 0, tb_rle = 0;
    HIPCHK(u64_sort(nullptr, tb_sort, dl, nullptr, n, h->stream));
    HIPCHK(u64_runs(nullptr, tb_rle, nullptr, nullptr, nullptr, nullptr, n, h->stream));
    if ((r = grow(h, h->rl_sorted, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->rl_uniq, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->rl_counts, sizeof(uint64_t) * (size_t)n + 64)) != CTWS_OK) return r;
    if ((r = grow(h, h->rl_tmp, std::max(tb_sort, tb_rle))) != CTWS_OK) return r;
    uint64_t* sorted = (uint64_t*)h->rl_sorted.p;
    uint64_t* uniq = (uint64_t*)h->rl_uniq.p;
    uint64_t* cnt = (uint64_t*)h->rl_counts.p;
    uint64_t* nruns = cnt + n;  // (the counts buffer has 64 spare bytes)
    HIPCHK(u64_sort(h->rl_tmp.p, tb_sort, dl, sorted, n, h->stream));
    HIPCHK(u64_runs(h->rl_tmp.p, tb_rle, sorted, uniq, cnt, nruns, n, h->stream));
    uint64_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, nruns, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *n_unique = (int64_t)total;
    if ((int64_t)total > cap) {
        h->err = "unique: output capacity too small";
        return CTWS_EINVAL;
    }
    const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (total) {
        HIPCHK(hipMemcpyAsync(out, uniq, sizeof(uint64_t) * total, k, h->stream));
        if (counts) HIPCHK(hipMemcpyAsync(counts, cnt, sizeof(uint64_t) * total, k, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTWS_OK;
}

const uint64_t* stage_labels(ctws_handle* h, const uint64_t* labels, int64_t n, int on_device, int* r) {
    *r = CTWS_OK;
    if (on_device) return labels;
    if ((*r = grow(h, h->rl_lab, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return nullptr;
    if (hipMemcpyAsync(h->rl_lab.p, labels, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream) !=
        hipSuccess) {
        h->err = "unique: label upload failed";
        *r = CTWS_EHIP;
        return nullptr;
    }
    return (const uint64_t*)h->rl_lab.p;
}
}  // namespace

extern "C" {

// ---- RelabelWorkflow kernels (k_relabel.hip) ----------------------------------------------
int ctws_unique_counts_u64(ctws_handle* h, const uint64_t* labels, int64_t n, int on_device, uint64_t* out,
                           uint64_t* counts, int64_t cap, int64_t* n_unique) {
    if (!h || (!labels && n > 0) || n < 0 || !n_unique || cap < 0 || ((!out || !counts) && cap > 0))
        return CTWS_EINVAL;
    h->err.clear();
    HIPCHK(hipSetDevice(h->device));
    *n_unique = 0;
    if (n == 0) return CTWS_OK;
    int r;
    const uint64_t* dl = stage_labels(h, labels, n, on_device, &r);
    if (r != CTWS_OK) return r;
    return unique_sorted(h, dl, n, on_device, out, counts, cap, n_unique);
}

int ctws_unique_u64(ctws_handle* h, const uint64_t* labels, int64_t n, int on_device, uint64_t* out, int64_t cap,
                    int64_t* n_unique) {
    if (!h || (!labels && n > 0) || n < 0 || !n_unique || cap < 0 || (!out && cap > 0)) return CTWS_EINVAL;
    h->err.clear();
    HIPCHK(hipSetDevice(h->device));
    *n_unique = 0;
    if (n == 0) return CTWS_OK;
    int r;
    const uint64_t* dl = stage_labels(h, labels, n, on_device, &r);
    if (r != CTWS_OK) return r;
    if ((r = grow(h, h->rl_red, 4 * sizeof(uint64_t))) != CTWS_OK) return r;
    unsigned long long* red = (unsigned long long*)h->rl_red.p;
    const unsigned long long init[3] = {~0ull, 0ull, 0ull};
    HIPCHK(hipMemcpyAsync(red, init, sizeof(init), hipMemcpyHostToDevice, h->stream));
    const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    k_u64_range<<<g, 256, 0, h->stream>>>(dl, n, red);
    LAUNCHCHK();
    unsigned long long hr[3];
    HIPCHK(hipMemcpyAsync(hr, red, sizeof(hr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const bool has_nz = hr[1] != 0ull;  // (the min stays ~0 when every nonzero label is 2^64 - 1)
    const int64_t first = hr[2] ? 1 : 0;
    int64_t total = first;
    if (has_nz) {
        const uint64_t lo = hr[0], span = hr[1] - hr[0];  // (+ 1 below; 0 .. 2^64 - 1 would wrap)
        // the bitmap (span / 8 bytes) only while it is no larger than sorting the labels would
        // need (~16 bytes each) or small anyway; otherwise sort (any value range)
        if (span >= (1ull << 35) || span / 64 + 1 > (uint64_t)std::max<int64_t>(2 * n, 1 << 20))
            return unique_sorted(h, dl, n, on_device, out, nullptr, cap, n_unique);
        const int64_t nw = (int64_t)(span / 64 + 1), nc = (nw + 255) / 256;
        if ((r = grow(h, h->rl_bits, sizeof(uint64_t) * (size_t)nw)) != CTWS_OK) return r;
        if ((r = grow(h, h->rl_cnt, sizeof(uint32_t) * (size_t)nc)) != CTWS_OK) return r;
        if ((r = grow(h, h->rl_offs, sizeof(uint64_t) * (size_t)(nc + 1))) != CTWS_OK) return r;
        HIPCHK(hipMemsetAsync(h->rl_bits.p, 0, sizeof(uint64_t) * (size_t)nw, h->stream));
        k_u64_bits<<<g, 256, 0, h->stream>>>(dl, n, lo, (unsigned long long*)h->rl_bits.p);
        k_bits_chunk_count<<<(unsigned)nc, 256, 0, h->stream>>>((const uint64_t*)h->rl_bits.p, nw,
                                                               (uint32_t*)h->rl_cnt.p);
        k_scan_chunks<<<1, 256, 0, h->stream>>>((const uint32_t*)h->rl_cnt.p, nc, (uint64_t*)h->rl_offs.p);
        LAUNCHCHK();
        uint64_t cnt = 0;
        HIPCHK(hipMemcpyAsync(&cnt, (uint64_t*)h->rl_offs.p + nc, sizeof(uint64_t), hipMemcpyDeviceToHost,
                              h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        total += (int64_t)cnt;
        *n_unique = total;
        if (total > cap) {
            h->err = "ctws_unique_u64: output capacity too small";
            return CTWS_EINVAL;
        }
        uint64_t* dout = out;
        if (!on_device) {
            if ((r = grow(h, h->rl_out, sizeof(uint64_t) * (size_t)total)) != CTWS_OK) return r;
            dout = (uint64_t*)h->rl_out.p;
        }
        k_bits_compact<<<(unsigned)nc, 256, 0, h->stream>>>((const uint64_t*)h->rl_bits.p, nw,
                                                           (const uint64_t*)h->rl_offs.p, lo, (uint64_t)first, dout);
        LAUNCHCHK();
        if (first) HIPCHK(hipMemsetAsync(dout, 0, sizeof(uint64_t), h->stream));
        if (!on_device)
            HIPCHK(hipMemcpyAsync(out, dout, sizeof(uint64_t) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        return CTWS_OK;
    }
    *n_unique = total;  // only zeros
    if (total > cap) {
        h->err = "ctws_unique_u64: output capacity too small";
        return CTWS_EINVAL;
    }
    if (on_device) HIPCHK(hipMemsetAsync(out, 0, sizeof(uint64_t), h->stream));
    else out[0] = 0;
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTWS_OK;
}

int ctws_set_table_u64(ctws_handle* h, const uint64_t* keys, const uint64_t* values, int64_t n_table) {
    if (!h || n_table < 0 || ((!keys || !values) && n_table > 0)) return CTWS_EINVAL;
    h->err.clear();
    HIPCHK(hipSetDevice(h->device));
    int r;
    if ((r = grow(h, h->rl_keys, sizeof(uint64_t) * (size_t)std::max<int64_t>(1, n_table))) != CTWS_OK) return r;
    if ((r = grow(h, h->rl_vals, sizeof(uint64_t) * (size_t)std::max<int64_t>(1, n_table))) != CTWS_OK) return r;
    if (n_table) {
        HIPCHK(hipMemcpyAsync(h->rl_keys.p, keys, sizeof(uint64_t) * (size_t)n_table, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->rl_vals.p, values, sizeof(uint64_t) * (size_t)n_table, hipMemcpyHostToDevice,
                              h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->rl_ntable = n_table;
    return CTWS_OK;
}

int ctws_lookup_u64(ctws_handle* h, uint64_t* labels, int64_t n, int on_device, const uint64_t* keys,
                    const uint64_t* values, int64_t n_table, int64_t* n_missing) {
    if (!h || (!labels && n > 0) || n < 0) return CTWS_EINVAL;
    const bool resident = !keys && !values;
    if (!resident && (n_table < 0 || ((!keys || !values) && n_table > 0))) return CTWS_EINVAL;
    h->err.clear();
    HIPCHK(hipSetDevice(h->device));
    if (n_missing) *n_missing = 0;
    if (n == 0) return CTWS_OK;
    int r;
    if (resident) {
        n_table = h->rl_ntable;
    } else if (!on_device) {
        // host table: upload it as the resident one
        if ((r = ctws_set_table_u64(h, keys, values, n_table)) != CTWS_OK) return r;
    }
    const uint64_t* dk = (resident || !on_device) ? (const uint64_t*)h->rl_keys.p : keys;
    const uint64_t* dv = (resident || !on_device) ? (const uint64_t*)h->rl_vals.p : values;
    uint64_t* dl = labels;
    if (!on_device) {
        if ((r = grow(h, h->rl_lab, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
        dl = (uint64_t*)h->rl_lab.p;
        HIPCHK(hipMemcpyAsync(dl, labels, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    }
    if ((r = grow(h, h->rl_red, 4 * sizeof(uint64_t))) != CTWS_OK) return r;
    unsigned long long* miss = (unsigned long long*)h->rl_red.p + 3;
    HIPCHK(hipMemsetAsync(miss, 0, sizeof(uint64_t), h->stream));
    const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    k_u64_lookup<<<g, 256, 0, h->stream>>>(dl, n, dk, dv, n_table, miss);
    LAUNCHCHK();
    unsigned long long hm = 0;
    HIPCHK(hipMemcpyAsync(&hm, miss, sizeof(hm), hipMemcpyDeviceToHost, h->stream));
    if (!on_device) HIPCHK(hipMemcpyAsync(labels, dl, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (n_missing) *n_missing = (int64_t)hm;
    return CTWS_OK;
}

// ---- the scaffold of the feature block calls below -------------------------------------------
extern "C++" {
namespace {
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

// the stage between events a and b of this call, in ms
void stage_time(ctws_handle* h, const char* name, size_t a, size_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->events[a], h->events[b]) == hipSuccess) add_timing(h, name, ms);
}

int call_begin(ctws_handle* h) {
    h->err.clear();
    h->timings.clear();
    HIPCHK(hipSetDevice(h->device));
    return CTWS_OK;
}

// the kernels index a block with 32 bits: every extent and product of extents stays below 2^31
int check_extent(ctws_handle* h, int64_t nz, int64_t ny, int64_t nx, const char* what, const char* unit,
                 const char* why) {
    constexpr int64_t kMax = 1ll << 31;
    if (nz >= kMax || ny >= kMax || nx >= kMax || nz * ny >= kMax || nz * ny * nx >= kMax) {
        h->err = std::string(what) + ": 2^31 or more voxels in one " + unit + " (" + why + ")";
        return CTWS_EUNSUPPORTED;
    }
    return CTWS_OK;
}

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

int out_end(ctws_handle* h, void* dst, const void* d, size_t bytes, bool dev) {
    if (!dev) HIPCHK(copy_pieces(dst, d, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTWS_OK;
}

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
unsigned long long first_cap(int64_t n, int64_t div) { return (unsigned long long)std::max<int64_t>(64, n / div); }

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
int runs_within(ctws_handle* h, const char* what, unsigned long long runs, int64_t lo, int64_t n) {
    if (runs >= (unsigned long long)lo && runs <= (unsigned long long)n) return CTWS_OK;
    h->err = std::string(what) + ": the kernel counted " + std::to_string(runs) + " runs in " + std::to_string(n) +
             " voxels";
    return CTWS_EHIP;
}

// Sort by id and run-length encode: n (id, record) pairs on the device -> the pairs sorted by id
// (rg_skeys, rg_sw) and the distinct ids with their numbers of pairs (rg_keys, rg_sum).  vmax: the
// largest id, for the sort's bits; the ids become float64 columns, so 2^53 or more is refused.
// ev: the event recorded behind the two launches.  The counters are those of rg_red.
struct ById {
    uint64_t *sids, *srecs, *uniq, *counts;
    int64_t m;  // the distinct ids
};
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
    HIPCHK(pair_sort(nullptr, tb_sort, nullptr, nullptr, nullptr, nullptr, n, bits, h->stream));
    HIPCHK(u64_runs(nullptr, tb_rle, nullptr, nullptr, nullptr, nullptr, n, h->stream));
    if ((r = grow(h, h->rg_skeys, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_sw, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_keys, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_sum, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_tmp, std::max(tb_sort, tb_rle))) != CTWS_OK) return r;
    o->sids = (uint64_t*)h->rg_skeys.p;
    o->srecs = (uint64_t*)h->rg_sw.p;
    o->uniq = (uint64_t*)h->rg_keys.p;
    o->counts = (uint64_t*)h->rg_sum.p;
    uint64_t* nruns = (uint64_t*)h->rg_red.p + kRedRuns;
    HIPCHK(pair_sort(h->rg_tmp.p, tb_sort, ids, o->sids, recs, o->srecs, n, bits, h->stream));
    HIPCHK(u64_runs(h->rg_tmp.p, tb_rle, o->sids, o->uniq, o->counts, nruns, n, h->stream));
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

// ---- GraphWorkflow: the region adjacency graph (k_rag.hip) ----------------------------------
// The sorted distinct values of dv (device) into rg_tab, by the relabel path's radix sort and
// run-length encoding: these are id tables with many repeats of few values over a narrow range,
// where the bitmap unique's atomics all land in a few words (57 ms for the 16.8 M labels of a
// block of fragments, measured).  The table grows to the size the first call reports.
int rag_table(ctws_handle* h, const uint64_t* dv, int64_t n, int64_t* nt) {
    int r;
    *nt = 0;
    if (n == 0) return CTWS_OK;
    const int64_t cap = std::max<int64_t>((int64_t)(h->rg_tab.bytes / sizeof(uint64_t)), 1 << 16);
    if ((r = grow(h, h->rg_tab, sizeof(uint64_t) * (size_t)cap)) != CTWS_OK) return r;
    r = unique_sorted(h, dv, n, 1, (uint64_t*)h->rg_tab.p, nullptr, cap, nt);
    if (r == CTWS_EINVAL && *nt > cap) {
        const int64_t want = *nt;
        h->err.clear();
        if ((r = grow(h, h->rg_tab, sizeof(uint64_t) * (size_t)want)) != CTWS_OK) return r;
        r = unique_sorted(h, dv, n, 1, (uint64_t*)h->rg_tab.p, nullptr, want, nt);
    }
    return r;
}

// The tail both entry points share: n (pair, weight) records on the device -> the sorted unique
// pairs in rg_out (m x 2) with their summed weights in rg_sum (m).  tab (device, ascending)
// holds every endpoint value; weights == nullptr counts 1 per record.
int pairs_tail(ctws_handle* h, const uint64_t* pairs, const uint64_t* weights, int64_t n, const uint64_t* tab,
               int64_t nt, int64_t* m) {
    *m = 0;
    if (n == 0) return CTWS_OK;
    if (n >= (1ll << 31)) {
        h->err = "unique pairs: more than 2^31 - 1 pairs in one call";
        return CTWS_EUNSUPPORTED;
    }
    if (nt >= (1ll << 32)) {
        h->err = "unique pairs: 2^32 or more distinct ids in one call (the sort keys hold two 32-bit ranks)";
        return CTWS_EUNSUPPORTED;
    }
    int b = 1;  // bits per rank
    while ((1ll << b) < nt) ++b;
    int r;
    const size_t nb = sizeof(uint64_t) * (size_t)n;
    size_t tb_sort = 0, tb_red = 0;
    HIPCHK(pair_sort(nullptr, tb_sort, nullptr, nullptr, nullptr, nullptr, n, 2 * b, h->stream));
    HIPCHK(pair_reduce(nullptr, tb_red, nullptr, nullptr, nullptr, nullptr, nullptr, n, h->stream));
    if ((r = grow(h, h->rg_keys, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_skeys, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_sw, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_sum, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_tmp, std::max(tb_sort, tb_red))) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_red, kRedWords * sizeof(uint64_t))) != CTWS_OK) return r;
    if (!weights && (r = grow(h, h->rg_w, nb)) != CTWS_OK) return r;
    uint64_t* keys = (uint64_t*)h->rg_keys.p;
    uint64_t* skeys = (uint64_t*)h->rg_skeys.p;
    uint64_t* sw = (uint64_t*)h->rg_sw.p;
    uint64_t* sums = (uint64_t*)h->rg_sum.p;
    unsigned long long* red = (unsigned long long*)h->rg_red.p;
    const unsigned g = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    HIPCHK(hipMemsetAsync(red + kRedPairRuns, 0, 2 * sizeof(uint64_t), h->stream));  // (and kRedPairMiss)
    record(h, 2);
    if (!weights) {
        k_pair_ones<<<g, 256, 0, h->stream>>>((uint64_t*)h->rg_w.p, n);
        weights = (const uint64_t*)h->rg_w.p;
    }
    k_pair_keys<<<g, 256, 0, h->stream>>>(pairs, n, tab, nt, b, keys, red + kRedPairMiss);
    LAUNCHCHK();
    record(h, 3);
    HIPCHK(pair_sort(h->rg_tmp.p, tb_sort, keys, skeys, weights, sw, n, 2 * b, h->stream));
    record(h, 4);
    // (the unsorted keys are dead: their buffer takes the unique keys)
    HIPCHK(pair_reduce(h->rg_tmp.p, tb_red, skeys, keys, sw, sums, (uint64_t*)(red + kRedPairRuns), n,
                       h->stream));
    record(h, 5);
    unsigned long long hr[2] = {0ull, 0ull};
    HIPCHK(hipMemcpyAsync(hr, red + kRedPairRuns, sizeof(hr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (hr[1]) {
        h->err = "unique pairs: " + std::to_string(hr[1]) + " endpoint values are missing from the id table";
        return CTWS_EINVAL;
    }
    *m = (int64_t)hr[0];
    if ((r = grow(h, h->rg_out, 2 * sizeof(uint64_t) * (size_t)*m)) != CTWS_OK) return r;
    const unsigned gm = (unsigned)std::min<int64_t>((*m + 255) / 256, 8192);
    k_pair_unpack<<<gm, 256, 0, h->stream>>>(keys, *m, tab, b, (uint64_t*)h->rg_out.p);
    LAUNCHCHK();
    record(h, 6);
    HIPCHK(hipStreamSynchronize(h->stream));
    stage_time(h, "pair_keys", 2, 3);
    stage_time(h, "pair_sort", 3, 4);
    stage_time(h, "pair_reduce", 4, 5);
    stage_time(h, "pair_unpack", 5, 6);
    return CTWS_OK;
}

// the tail's result -> the caller's buffers (the sizes are known to fit)
int pairs_out(ctws_handle* h, int64_t m, int on_device, uint64_t* out, uint64_t* counts) {
    if (m) {
        const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        HIPCHK(hipMemcpyAsync(out, h->rg_out.p, 2 * sizeof(uint64_t) * (size_t)m, k, h->stream));
        if (counts) HIPCHK(hipMemcpyAsync(counts, h->rg_sum.p, sizeof(uint64_t) * (size_t)m, k, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return CTWS_OK;
}

int rag_block(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx, int ignore_label,
              uint64_t* nodes, int64_t cap_nodes, int64_t* n_nodes, uint64_t* edges, uint64_t* counts,
              int64_t cap_edges, int64_t* n_edges, bool dev) {
    if (!h || !labels || nz <= 0 || ny <= 0 || nx <= 0 || !n_nodes || !n_edges || cap_nodes < 0 || cap_edges < 0 ||
        (!nodes && cap_nodes > 0) || (!edges && cap_edges > 0))
        return CTWS_EINVAL;
    int r;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    *n_nodes = *n_edges = 0;
    r = check_extent(h, nz, ny, nx, "rag block", "block", "the pair kernel indexes a block with 32 bits");
    if (r != CTWS_OK) return r;
    const int64_t N = nz * ny * nx;
    const uint64_t* dl;
    if ((r = stage_in(h, h->rg_lab, labels, sizeof(uint64_t) * (size_t)N, dev, &dl)) != CTWS_OK) return r;
    // one pass emits the pairs and the node ids, into first buffers of a quarter / a sixteenth of
    // the voxels
    if ((r = grow(h, h->rg_red, kRedWords * sizeof(uint64_t))) != CTWS_OK) return r;
    unsigned long long* cnt = (unsigned long long*)h->rg_red.p;
    RagArgs a;
    a.lab = dl;
    a.nz = (uint32_t)nz;
    a.ny = (uint32_t)ny;
    a.nx = (uint32_t)nx;
    a.ignore = ignore_label ? 1 : 0;
    a.count = cnt;
    a.ncount = cnt + kRedNodes;
    const int64_t rows = nz * ny;
    // four workgroups per CU (their LDS stages) and no more: every wave ends with an append of
    // its own, and one counter word takes only ~85 returning atomics per microsecond
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, 1024));
    EmitCap caps[2] = {{kRedEmit, first_cap(N, 4)}, {kRedNodes, first_cap(N, 16)}};
    Emitted e;
    record(h, 0);
    r = counted_emit(
        h, "rag block", cnt, kRedNodes + 1, kRedNodes + 1, caps, 2,
        [&] {
            int r;
            if ((r = grow(h, h->rg_pairs, 2 * sizeof(uint64_t) * (size_t)caps[0].cap)) != CTWS_OK) return r;
            if ((r = grow(h, h->rg_w, sizeof(uint64_t) * (size_t)caps[0].cap)) != CTWS_OK) return r;
            if ((r = grow(h, h->rg_nodes, sizeof(uint64_t) * (size_t)caps[1].cap)) != CTWS_OK) return r;
            a.pairs = (uint64_t*)h->rg_pairs.p;
            a.weights = (uint64_t*)h->rg_w.p;
            a.nodes = (uint64_t*)h->rg_nodes.p;
            a.cap = caps[0].cap;
            a.ncap = caps[1].cap;
            k_rag_pairs<<<g, 256, 0, h->stream>>>(a);
            return CTWS_OK;
        },
        [](const unsigned long long*) { return CTWS_OK; }, &e);
    if (r != CTWS_OK) return r;
    const int64_t n_pairs = (int64_t)e.w[kRedEmit], n_ids = (int64_t)e.w[kRedNodes];
    record(h, 1);
    // nodes: the sorted unique of the emitted ids = np.unique of the block (without 0 under
    // ignore_label: the kernel emits no 0 then)
    int64_t nt = 0;
    if ((r = rag_table(h, (const uint64_t*)h->rg_nodes.p, n_ids, &nt)) != CTWS_OK) return r;
    const uint64_t* tab = (const uint64_t*)h->rg_tab.p;
    record(h, 7);
    HIPCHK(hipStreamSynchronize(h->stream));
    stage_time(h, "rag_pairs", 0, 1);
    stage_time(h, "rag_nodes", 1, 7);
    add_timing(h, "rag_pair_passes", (float)e.passes);  // (counts, as the flood's rounds)
    add_timing(h, "rag_emits", (float)n_pairs);
    add_timing(h, "rag_node_emits", (float)n_ids);
    int64_t m = 0;
    if ((r = pairs_tail(h, (const uint64_t*)h->rg_pairs.p, (const uint64_t*)h->rg_w.p, n_pairs, tab, nt, &m)) !=
        CTWS_OK)
        return r;
    *n_nodes = nt;
    *n_edges = m;
    if (*n_nodes > cap_nodes || m > cap_edges) {
        h->err = "rag block: output capacity too small";
        return CTWS_EINVAL;
    }
    if (*n_nodes)
        HIPCHK(hipMemcpyAsync(nodes, tab, sizeof(uint64_t) * (size_t)*n_nodes,
                              dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    return pairs_out(h, m, dev ? 1 : 0, edges, counts);
}
}  // namespace
}  // extern "C++"

int ctws_unique_pairs_u64(ctws_handle* h, const uint64_t* pairs, const uint64_t* weights, int64_t n, int on_device,
                          uint64_t* out, uint64_t* counts, int64_t cap, int64_t* n_unique) {
    if (!h || (!pairs && n > 0) || n < 0 || !n_unique || cap < 0 || (!out && cap > 0)) return CTWS_EINVAL;
    int r;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    *n_unique = 0;
    if (n == 0) return CTWS_OK;
    if (n >= (1ll << 30)) {
        h->err = "unique pairs: 2^30 or more pairs in one call";
        return CTWS_EUNSUPPORTED;
    }
    const bool dev = on_device != 0;
    if ((r = stage_in(h, h->rg_pairs, pairs, 2 * sizeof(uint64_t) * (size_t)n, dev, &pairs)) != CTWS_OK) return r;
    if (weights && (r = stage_in(h, h->rg_lab, weights, sizeof(uint64_t) * (size_t)n, dev, &weights)) != CTWS_OK)
        return r;
    // ids -> ranks: the distinct endpoint values
    int64_t nt = 0;
    if ((r = rag_table(h, pairs, 2 * n, &nt)) != CTWS_OK) return r;
    int64_t m = 0;
    if ((r = pairs_tail(h, pairs, weights, n, (const uint64_t*)h->rg_tab.p, nt, &m)) != CTWS_OK) return r;
    *n_unique = m;
    if (m > cap) {
        h->err = "ctws_unique_pairs_u64: output capacity too small";
        return CTWS_EINVAL;
    }
    return pairs_out(h, m, on_device, out, counts);
}

int ctws_rag_block(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx, int ignore_label,
                   uint64_t* nodes, int64_t cap_nodes, int64_t* n_nodes, uint64_t* edges, uint64_t* counts,
                   int64_t cap_edges, int64_t* n_edges) {
    return rag_block(h, labels, nz, ny, nx, ignore_label, nodes, cap_nodes, n_nodes, edges, counts, cap_edges, n_edges,
                     false);
}

int ctws_rag_block_device(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx, int ignore_label,
                          uint64_t* nodes, int64_t cap_nodes, int64_t* n_nodes, uint64_t* edges, uint64_t* counts,
                          int64_t cap_edges, int64_t* n_edges) {
    return rag_block(h, labels, nz, ny, nx, ignore_label, nodes, cap_nodes, n_nodes, edges, counts, cap_edges, n_edges,
                     true);
}


// ---- NodeLabelWorkflow: fragment / label overlaps (k_overlaps.hip) ---------------------------
extern "C++" {
namespace {
int label_overlaps(ctws_handle* h, const uint64_t* nodes_vol, const uint64_t* labels_vol, int64_t n, int with_ignore,
                   uint64_t ignore_label, uint64_t* rows, int64_t cap, int64_t* n_rows, bool dev) {
    if (!h || n < 0 || ((!nodes_vol || !labels_vol) && n > 0) || !n_rows || cap < 0 || (!rows && cap > 0))
        return CTWS_EINVAL;
    int r;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    *n_rows = 0;
    if (n == 0) return CTWS_OK;
    r = check_extent(h, 1, 1, n, "label overlaps", "call", "the pair kernel indexes the arrays with 32 bits");
    if (r != CTWS_OK) return r;
    const size_t nb = sizeof(uint64_t) * (size_t)n;
    const uint64_t *dn, *dl;
    if ((r = stage_in(h, h->rg_lab, nodes_vol, nb, dev, &dn)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->ov_lab, labels_vol, nb, dev, &dl)) != CTWS_OK) return r;
    // the run heads, at most one per voxel, into a first buffer of a quarter of the voxels
    if ((r = grow(h, h->rg_red, kRedWords * sizeof(uint64_t))) != CTWS_OK) return r;
    unsigned long long* cnt = (unsigned long long*)h->rg_red.p;
    OvArgs a;
    a.nodes = dn;
    a.labels = dl;
    a.n = (uint32_t)n;
    a.with_ignore = with_ignore ? 1 : 0;
    a.ignore_label = ignore_label;
    a.count = cnt;
    const int64_t words = (n + 63) / 64;
    // four workgroups per CU, as k_rag_pairs: every wave ends with an append of its own
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((words + 3) / 4, 1024));
    EmitCap ecap = {kRedEmit, first_cap(n, 4)};
    Emitted e;
    record(h, 0);
    r = counted_emit(
        h, "label overlaps", cnt, 1, 1, &ecap, 1,
        [&] {
            int r;
            if ((r = grow(h, h->rg_pairs, 2 * sizeof(uint64_t) * (size_t)ecap.cap)) != CTWS_OK) return r;
            if ((r = grow(h, h->rg_w, sizeof(uint64_t) * (size_t)ecap.cap)) != CTWS_OK) return r;
            a.pairs = (uint64_t*)h->rg_pairs.p;
            a.weights = (uint64_t*)h->rg_w.p;
            a.cap = ecap.cap;
            k_ov_pairs<<<g, 256, 0, h->stream>>>(a);
            return CTWS_OK;
        },
        [&](const unsigned long long* w) { return runs_within(h, "label overlaps", w[kRedEmit], 0, n); }, &e);
    if (r != CTWS_OK) return r;
    const unsigned long long emitted = e.w[kRedEmit];
    record(h, 1);
    HIPCHK(hipStreamSynchronize(h->stream));
    stage_time(h, "ov_pairs", 0, 1);
    add_timing(h, "ov_pair_passes", (float)e.passes);  // (counts, as the flood's rounds)
    add_timing(h, "ov_emits", (float)emitted);
    if (emitted == 0) return CTWS_OK;  // every voxel carries the ignore label
    if (emitted >= (1ull << 30)) {
        h->err = "label overlaps: 2^30 or more runs of equal (node, label) pairs in one call";
        return CTWS_EUNSUPPORTED;
    }
    // ids -> ranks in one table for both sides: the key order is the (node, label) order
    int64_t nt = 0, m = 0;
    if ((r = rag_table(h, (const uint64_t*)h->rg_pairs.p, 2 * (int64_t)emitted, &nt)) != CTWS_OK) return r;
    record(h, 7);
    HIPCHK(hipStreamSynchronize(h->stream));
    stage_time(h, "ov_table", 1, 7);
    if ((r = pairs_tail(h, (const uint64_t*)h->rg_pairs.p, (const uint64_t*)h->rg_w.p, (int64_t)emitted,
                        (const uint64_t*)h->rg_tab.p, nt, &m)) != CTWS_OK)
        return r;
    *n_rows = m;
    if (m > cap) {
        h->err = "label overlaps: output capacity too small";
        return CTWS_EINVAL;
    }
    const size_t rb = 3 * sizeof(uint64_t) * (size_t)m;
    uint64_t* drows;
    if ((r = out_begin(h, h->ov_rows, rows, rb, dev, &drows)) != CTWS_OK) return r;
    const unsigned gm = (unsigned)std::min<int64_t>((m + 255) / 256, 8192);
    k_ov_rows<<<gm, 256, 0, h->stream>>>((const uint64_t*)h->rg_out.p, (const uint64_t*)h->rg_sum.p, m, drows);
    LAUNCHCHK();
    return out_end(h, rows, drows, rb, dev);
}
}  // namespace
}  // extern "C++"

int ctws_label_overlaps(ctws_handle* h, const uint64_t* nodes_vol, const uint64_t* labels_vol, int64_t n,
                        int with_ignore, uint64_t ignore_label, uint64_t* rows, int64_t cap, int64_t* n_rows) {
    return label_overlaps(h, nodes_vol, labels_vol, n, with_ignore, ignore_label, rows, cap, n_rows, false);
}

int ctws_label_overlaps_device(ctws_handle* h, const uint64_t* nodes_vol, const uint64_t* labels_vol, int64_t n,
                               int with_ignore, uint64_t ignore_label, uint64_t* rows, int64_t cap, int64_t* n_rows) {
    return label_overlaps(h, nodes_vol, labels_vol, n, with_ignore, ignore_label, rows, cap, n_rows, true);
}

// ---- MorphologyWorkflow: size, centre and bounding box per id (k_morph.hip) ------------------
extern "C++" {
namespace {
int block_morphology(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx, const int64_t* begin,
                     double* rows, int64_t cap, int64_t* n_rows, bool dev) {
    if (!h || !labels || nz <= 0 || ny <= 0 || nx <= 0 || !begin || !n_rows || cap < 0 || (!rows && cap > 0))
        return CTWS_EINVAL;
    int r;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    *n_rows = 0;
    if (begin[0] < 0 || begin[1] < 0 || begin[2] < 0) {
        h->err = "block morphology: a negative begin";
        return CTWS_EINVAL;
    }
    // the record packs z, y, x0 into 19 bits each; begin + extent <= 2^21 and fewer than 2^31
    // voxels keep every coordinate sum below 2^52, exact in a double
    constexpr int64_t kExt = 1ll << 19, kCoord = 1ll << 21;
    if (nz >= kExt || ny >= kExt || nx >= kExt) {
        h->err = "block morphology: an extent of 2^19 or more (the run record holds 19 bits per coordinate)";
        return CTWS_EUNSUPPORTED;
    }
    r = check_extent(h, nz, ny, nx, "block morphology", "block", "the run kernel indexes a block with 32 bits");
    if (r != CTWS_OK) return r;
    const int64_t ext[3] = {nz, ny, nx};
    for (int d = 0; d < 3; ++d)
        if (begin[d] > kCoord || begin[d] + ext[d] > kCoord) {
            h->err = "block morphology: begin + extent above 2^21 (the coordinate sums would not be exact doubles)";
            return CTWS_EUNSUPPORTED;
        }
    const int64_t N = nz * ny * nx;
    const uint64_t* dl;
    if ((r = stage_in(h, h->rg_lab, labels, sizeof(uint64_t) * (size_t)N, dev, &dl)) != CTWS_OK) return r;
    // the run heads, at least one and at most one per voxel, into a first buffer of a quarter of
    // the voxels
    if ((r = grow(h, h->rg_red, kRedWords * sizeof(uint64_t))) != CTWS_OK) return r;
    unsigned long long* cnt = (unsigned long long*)h->rg_red.p;
    MorphArgs a;
    a.lab = dl;
    a.nz = (uint32_t)nz;
    a.ny = (uint32_t)ny;
    a.nx = (uint32_t)nx;
    a.count = cnt;
    a.vmax = cnt + kRedVmax;
    const int64_t lines = nz * ny;
    // four workgroups per CU, as k_rag_pairs: every wave ends with an append of its own
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((lines + 3) / 4, 1024));
    EmitCap ecap = {kRedEmit, first_cap(N, 4)};
    Emitted e;
    record(h, 0);
    r = counted_emit(
        h, "block morphology", cnt, kRedVmax + 1, kRedVmax + 1, &ecap, 1,
        [&] {
            int r;
            if ((r = grow(h, h->rg_pairs, sizeof(uint64_t) * (size_t)ecap.cap)) != CTWS_OK) return r;
            if ((r = grow(h, h->rg_w, sizeof(uint64_t) * (size_t)ecap.cap)) != CTWS_OK) return r;
            a.ids = (uint64_t*)h->rg_pairs.p;
            a.recs = (uint64_t*)h->rg_w.p;
            a.cap = ecap.cap;
            k_morph_runs<<<g, 256, 0, h->stream>>>(a);
            return CTWS_OK;
        },
        [&](const unsigned long long* w) { return runs_within(h, "block morphology", w[kRedEmit], 1, N); }, &e);
    if (r != CTWS_OK) return r;
    const int64_t n = (int64_t)e.w[kRedEmit];  // (< 2^31)
    record(h, 1);
    // the largest id was taken by the run pass
    ById s;
    if ((r = sort_by_id(h, "block morphology", a.ids, a.recs, n, e.w[kRedVmax], 2, &s)) != CTWS_OK) return r;
    stage_time(h, "morph_runs", 0, 1);
    stage_time(h, "morph_sort", 1, 2);
    add_timing(h, "morph_run_passes", (float)e.passes);  // (counts, as the flood's rounds)
    add_timing(h, "morph_emits", (float)n);
    const int64_t m = s.m;
    *n_rows = m;
    if (m > cap) {
        h->err = "block morphology: output capacity too small";
        return CTWS_EINVAL;
    }
    const size_t rb = 11 * sizeof(double) * (size_t)m;
    double* drows;
    if ((r = out_begin(h, h->mo_rows, rows, rb, dev, &drows)) != CTWS_OK) return r;
    // the per-id table of the split segments: ten integers per id, zero = neutral
    const size_t ab = 10 * sizeof(uint64_t) * (size_t)m;
    if ((r = grow(h, h->mo_acc, ab)) != CTWS_OK) return r;
    unsigned long long* acc = (unsigned long long*)h->mo_acc.p;
    HIPCHK(hipMemsetAsync(acc, 0, ab, h->stream));
    const MorphBegin b = {(uint64_t)begin[0], (uint64_t)begin[1], (uint64_t)begin[2]};
    const int64_t waves = m + n / kMorphChunk;  // a wave per id and per whole chunk of records
    const unsigned gm = (unsigned)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, 2048));
    k_morph_rows<<<gm, 256, 0, h->stream>>>(s.sids, s.srecs, (uint32_t)n, s.uniq, s.counts, (uint32_t)m, b, acc, drows);
    LAUNCHCHK();
    if (n >= (int64_t)kMorphChunk) {  // (a shorter record list holds no whole chunk: no split segment)
        const unsigned gl = (unsigned)std::min<int64_t>((m + 255) / 256, 1024);
        k_morph_long_rows<<<gl, 256, 0, h->stream>>>(s.uniq, (uint32_t)m, b, acc, drows);
        LAUNCHCHK();
    }
    record(h, 3);
    if ((r = out_end(h, rows, drows, rb, dev)) != CTWS_OK) return r;
    stage_time(h, "morph_rows", 2, 3);
    return CTWS_OK;
}
}  // namespace
}  // extern "C++"

int ctws_block_morphology(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx,
                          const int64_t begin[3], double* rows, int64_t cap, int64_t* n_rows) {
    return block_morphology(h, labels, nz, ny, nx, begin, rows, cap, n_rows, false);
}

int ctws_block_morphology_device(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx,
                                 const int64_t begin[3], double* rows, int64_t cap, int64_t* n_rows) {
    return block_morphology(h, labels, nz, ny, nx, begin, rows, cap, n_rows, true);
}

// ---- RegionFeaturesWorkflow: count and mean input value per id (k_regfeat.hip) --------------
extern "C++" {
namespace {
int region_features_block(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype, int64_t nz,
                          int64_t ny, int64_t nx, int with_ignore, uint64_t ignore_label, double* rows, int64_t cap,
                          int64_t* n_rows, bool dev) {
    if (!h || !labels || !data || nz <= 0 || ny <= 0 || nx <= 0 || !n_rows || cap < 0 || (!rows && cap > 0))
        return CTWS_EINVAL;
    int r;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    *n_rows = 0;
    if (data_dtype != CTWS_U8 && data_dtype != CTWS_U16 && data_dtype != CTWS_F32 && data_dtype != CTWS_F64) {
        h->err = "region features: the input map is uint8, uint16, float32 or float64";
        return CTWS_EINVAL;
    }
    r = check_extent(h, nz, ny, nx, "region features", "block", "the kernels index a block with 32 bits");
    if (r != CTWS_OK) return r;
    const int64_t N = nz * ny * nx, lines = nz * ny;
    if (lines + 1 >= (1ll << 31)) {  // (the scan takes the rows' counts and one 0 behind them with a 32-bit size)
        h->err = "region features: 2^31 - 1 rows in one block (the scan of the rows' run counts is 32-bit)";
        return CTWS_EUNSUPPORTED;
    }
    const size_t es = data_dtype == CTWS_U8 ? 1 : data_dtype == CTWS_U16 ? 2 : data_dtype == CTWS_F32 ? 4 : 8;
    const uint64_t* dl;
    const void* dd;
    if ((r = stage_in(h, h->rg_lab, labels, sizeof(uint64_t) * (size_t)N, dev, &dl)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->rf_data, data, es * (size_t)N, dev, &dd)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_red, kRedWords * sizeof(uint64_t))) != CTWS_OK) return r;
    unsigned long long* red = (unsigned long long*)h->rg_red.p;
    // the rows' run counts with one 0 behind them: the scan's last entry is the total
    const size_t cb = sizeof(uint32_t) * (size_t)(lines + 1);
    size_t tb_scan = 0;
    HIPCHK(u32_exclusive_sum(nullptr, tb_scan, nullptr, nullptr, lines + 1, h->stream));
    if ((r = grow(h, h->rf_cnt, cb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rf_off, cb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_tmp, tb_scan)) != CTWS_OK) return r;
    uint32_t* rcnt = (uint32_t*)h->rf_cnt.p;
    uint32_t* roff = (uint32_t*)h->rf_off.p;
    // four workgroups per CU, a wave per row
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((lines + 3) / 4, 1024));
    record(h, 0);
    HIPCHK(hipMemsetAsync(rcnt + lines, 0, sizeof(uint32_t), h->stream));
    HIPCHK(hipMemsetAsync(red, 0, kRedWords * sizeof(uint64_t), h->stream));
    k_regfeat_count<<<g, 256, 0, h->stream>>>(dl, (uint32_t)lines, (uint32_t)nx, rcnt);
    LAUNCHCHK();
    HIPCHK(u32_exclusive_sum(h->rg_tmp.p, tb_scan, rcnt, roff, lines + 1, h->stream));
    record(h, 1);
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, roff + lines, sizeof(total), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (total == 0 || (int64_t)total > N) {
        h->err = "region features: the count kernel found " + std::to_string(total) + " runs";
        return CTWS_EHIP;
    }
    const int64_t n = (int64_t)total;  // (< 2^31): the record arrays hold exactly the runs
    const size_t nb = sizeof(uint64_t) * (size_t)n;
    if ((r = grow(h, h->rg_pairs, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rg_w, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->rf_sums, sizeof(double) * (size_t)n)) != CTWS_OK) return r;
    RegfeatArgs a;
    a.lab = dl;
    a.data = dd;
    a.rows = (uint32_t)lines;
    a.nx = (uint32_t)nx;
    a.with_ignore = with_ignore ? 1 : 0;
    a.ignore = ignore_label;
    a.row_first = roff;
    a.n = total;
    a.ids = (uint64_t*)h->rg_pairs.p;
    a.vals = (uint64_t*)h->rg_w.p;
    a.sums = (double*)h->rf_sums.p;
    a.vmax = red + kRedVmax;
    if (data_dtype == CTWS_U8) k_regfeat_runs<uint8_t><<<g, 256, 0, h->stream>>>(a);
    else if (data_dtype == CTWS_U16) k_regfeat_runs<uint16_t><<<g, 256, 0, h->stream>>>(a);
    else if (data_dtype == CTWS_F32) k_regfeat_runs<float><<<g, 256, 0, h->stream>>>(a);
    else k_regfeat_runs<double><<<g, 256, 0, h->stream>>>(a);
    LAUNCHCHK();
    record(h, 2);
    unsigned long long vmax = 0;  // the largest id
    HIPCHK(hipMemcpyAsync(&vmax, red + kRedVmax, sizeof(vmax), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    ById s;
    if ((r = sort_by_id(h, "region features", a.ids, a.vals, n, vmax, 3, &s)) != CTWS_OK) return r;
    stage_time(h, "regfeat_count", 0, 1);
    stage_time(h, "regfeat_runs", 1, 2);
    stage_time(h, "regfeat_sort", 2, 3);
    add_timing(h, "regfeat_records", (float)total);  // (a count, as the flood's rounds)
    const int64_t m = s.m;
    *n_rows = m;
    if (m > cap) {
        h->err = "region features: output capacity too small";
        return CTWS_EINVAL;
    }
    const size_t rb = 3 * sizeof(double) * (size_t)m;
    double* drows;
    if ((r = out_begin(h, h->rf_rows, rows, rb, dev, &drows)) != CTWS_OK) return r;
    // the chunk table: (n, sum) per whole aligned chunk of sorted records, the n first
    const int64_t chunks = n / kRegfeatChunk;
    if ((r = grow(h, h->rf_ctab, 2 * sizeof(uint64_t) * (size_t)std::max<int64_t>(1, chunks))) != CTWS_OK) return r;
    uint64_t* chunk_n = (uint64_t*)h->rf_ctab.p;
    double* chunk_s = (double*)(chunk_n + std::max<int64_t>(1, chunks));
    if (chunks > 0) {
        const unsigned gc = (unsigned)std::min<int64_t>((chunks + 3) / 4, 2048);
        k_regfeat_chunks<<<gc, 256, 0, h->stream>>>(s.sids, s.srecs, a.sums, total, chunk_n, chunk_s);
        LAUNCHCHK();
    }
    const unsigned gm = (unsigned)std::max<int64_t>(1, std::min<int64_t>((m + 3) / 4, 2048));
    k_regfeat_rows<<<gm, 256, 0, h->stream>>>(s.sids, s.srecs, a.sums, total, s.uniq, s.counts, (uint32_t)m, chunk_n,
                                              chunk_s, drows);
    LAUNCHCHK();
    record(h, 4);
    if ((r = out_end(h, rows, drows, rb, dev)) != CTWS_OK) return r;
    stage_time(h, "regfeat_rows", 3, 4);
    return CTWS_OK;
}
}  // namespace
}  // extern "C++"

int ctws_region_features_block(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype, int64_t nz,
                               int64_t ny, int64_t nx, int with_ignore, uint64_t ignore_label, double* rows,
                               int64_t cap, int64_t* n_rows) {
    return region_features_block(h, labels, data, data_dtype, nz, ny, nx, with_ignore, ignore_label, rows, cap,
                                 n_rows, false);
}

int ctws_region_features_block_device(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype,
                                      int64_t nz, int64_t ny, int64_t nx, int with_ignore, uint64_t ignore_label,
                                      double* rows, int64_t cap, int64_t* n_rows) {
    return region_features_block(h, labels, data, data_dtype, nz, ny, nx, with_ignore, ignore_label, rows, cap,
                                 n_rows, true);
}

// ---- DownscalingWorkflow: block reduction of one block (k_downscale.hip) ---------------------
extern "C++" {
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
}  // extern "C++"

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

// ---- ImageFilter: Gaussian derivative filters of one block (k_imgfilter.hip) -----------------
extern "C++" {
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
}  // extern "C++"

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

// ---- RegionCentersWorkflow: the voxel farthest from the border per object (k_regcenter.hip) ---
extern "C++" {
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
}  // extern "C++"

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

// ---- EdgeFeaturesWorkflow: boundary-map statistics per edge (k_edgefeat.hip) ----------------
extern "C++" {
namespace {
int edge_features_block(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype, int64_t nz,
                        int64_t ny, int64_t nx, int64_t cz, int64_t cy, int64_t cx, int ignore_label,
                        const uint64_t* nodes, int64_t n_nodes, const uint64_t* edges, int64_t n_edges, double* out,
                        int64_t* n_missing, bool dev) {
    int r;
    if (!h) return CTWS_EINVAL;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    if (n_missing) *n_missing = 0;
    if (!labels || !data || nz <= 0 || ny <= 0 || nx <= 0 || cz <= 0 || cy <= 0 || cx <= 0 || cz > nz || cy > ny ||
        cx > nx || n_nodes < 0 || n_edges < 0 || (n_edges > 0 && (!nodes || !edges || !out || n_nodes == 0))) {
        h->err = "edge features: bad arguments (3-D boxes with 0 < core <= extended, tables for n_edges > 0)";
        return CTWS_EINVAL;
    }
    if (data_dtype != CTWS_F32 && data_dtype != CTWS_U8) {
        h->err = "edge features: the boundary map is float32 or uint8";
        return CTWS_EUNSUPPORTED;
    }
    if (n_edges == 0) return CTWS_OK;  // nothing to accumulate into: no launch
    r = check_extent(h, nz, ny, nx, "edge features", "block", "the sample kernel indexes a block with 32 bits");
    if (r != CTWS_OK) return r;
    if (n_nodes >= (1ll << 32) || n_edges >= (1ll << 32)) {
        h->err = "edge features: 2^32 or more nodes or edges in one block";
        return CTWS_EUNSUPPORTED;
    }
    const int64_t N = nz * ny * nx;
    const size_t es = data_dtype == CTWS_U8 ? 1 : 4;
    const uint64_t *dl, *dn, *de;
    const void* dd;
    double* dout;
    const size_t out_bytes = 10 * sizeof(double) * (size_t)n_edges;
    if ((r = stage_in(h, h->ef_lab, labels, sizeof(uint64_t) * (size_t)N, dev, &dl)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->ef_data, data, es * (size_t)N, dev, &dd)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->ef_nodes, nodes, sizeof(uint64_t) * (size_t)n_nodes, dev, &dn)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->ef_edges, edges, 2 * sizeof(uint64_t) * (size_t)n_edges, dev, &de)) != CTWS_OK) return r;
    if ((r = out_begin(h, h->ef_out, out, out_bytes, dev, &dout)) != CTWS_OK) return r;
    int b = 1;  // bits per rank
    while ((1ll << b) < n_nodes) ++b;
    int eb = 1;  // bits per edge index
    while ((1ll << eb) < n_edges) ++eb;
    if ((r = grow(h, h->ef_red, kRedWords * sizeof(uint64_t))) != CTWS_OK) return r;
    if ((r = grow(h, h->ef_ekeys, sizeof(uint64_t) * (size_t)n_edges)) != CTWS_OK) return r;
    unsigned long long* cnt = (unsigned long long*)h->ef_red.p;
    HIPCHK(hipMemsetAsync(cnt, 0, kRedWords * sizeof(uint64_t), h->stream));
    record(h, 0);
    const unsigned ge = (unsigned)std::min<int64_t>((n_edges + 255) / 256, 8192);
    k_ef_edge_keys<<<ge, 256, 0, h->stream>>>(de, n_edges, dn, n_nodes, b, (uint64_t*)h->ef_ekeys.p,
                                              cnt + kRedBadEdges);
    LAUNCHCHK();
    record(h, 1);
    EfArgs a;
    a.lab = dl;
    a.data = dd;
    a.nz = (uint32_t)nz;
    a.ny = (uint32_t)ny;
    a.nx = (uint32_t)nx;
    a.cz = (uint32_t)cz;
    a.cy = (uint32_t)cy;
    a.cx = (uint32_t)cx;
    a.ignore = ignore_label ? 1 : 0;
    a.tab = dn;
    a.nt = (uint32_t)n_nodes;
    a.b = b;
    a.ekeys = (const uint64_t*)h->ef_ekeys.p;
    a.ne = (uint32_t)n_edges;
    a.count = cnt;
    a.missing = cnt + kRedMissing;
    const int64_t rows = cz * cy;
    // the grid of k_rag_pairs: four workgroups per CU, every wave ends with an append of its own
    const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows + 3) / 4, 1024));
    // first capacity: half a key per voxel (a block of fragments emits ~0.38).  The bad-edge
    // count of k_ef_edge_keys is read with the pass's own counters, and not zeroed with them
    EmitCap ecap = {kRedEmit, first_cap(N, 2)};
    Emitted e;
    r = counted_emit(
        h, "edge features", cnt, kRedMissing + 1, kRedBadEdges + 1, &ecap, 1,
        [&] {
            const int r = grow(h, h->ef_keys, sizeof(uint64_t) * (size_t)ecap.cap);
            if (r != CTWS_OK) return r;
            a.keys = (uint64_t*)h->ef_keys.p;
            a.cap = ecap.cap;
            if (data_dtype == CTWS_U8) k_ef_samples<uint8_t><<<g, 256, 0, h->stream>>>(a);
            else k_ef_samples<float><<<g, 256, 0, h->stream>>>(a);
            return CTWS_OK;
        },
        [&](const unsigned long long* w) {
            if (!w[kRedBadEdges]) return CTWS_OK;
            h->err = "edge features: " + std::to_string(w[kRedBadEdges]) +
                     " edges have an endpoint missing from the nodes or are not sorted and unique";
            return CTWS_EINVAL;
        },
        &e);
    if (r != CTWS_OK) return r;
    record(h, 2);
    const int64_t n = (int64_t)e.w[kRedEmit];
    if (n >= (1ll << 31)) {
        h->err = "edge features: 2^31 or more samples in one block";
        return CTWS_EUNSUPPORTED;
    }
    if (n_missing) *n_missing = (int64_t)e.w[kRedMissing];
    const uint64_t* sorted = (const uint64_t*)h->ef_keys.p;
    if (n) {
        size_t tb = 0;
        HIPCHK(ef_sort(nullptr, tb, nullptr, nullptr, n, 32 + eb, h->stream));
        if ((r = grow(h, h->ef_skeys, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
        if ((r = grow(h, h->ef_tmp, tb)) != CTWS_OK) return r;
        HIPCHK(ef_sort(h->ef_tmp.p, tb, (const uint64_t*)h->ef_keys.p, (uint64_t*)h->ef_skeys.p, n, 32 + eb,
                       h->stream));
        sorted = (const uint64_t*)h->ef_skeys.p;
    }
    record(h, 3);
    // one wave per edge, four per workgroup
    k_ef_stats<<<(unsigned)((n_edges + 3) / 4), 256, 0, h->stream>>>(sorted, (uint32_t)n, (uint32_t)n_edges, dout);
    LAUNCHCHK();
    record(h, 4);
    if ((r = out_end(h, out, dout, out_bytes, dev)) != CTWS_OK) return r;
    stage_time(h, "ef_edge_keys", 0, 1);
    stage_time(h, "ef_samples", 1, 2);
    stage_time(h, "ef_sort", 2, 3);
    stage_time(h, "ef_stats", 3, 4);
    add_timing(h, "ef_sample_passes", (float)e.passes);
    add_timing(h, "ef_keys", (float)n);
    return CTWS_OK;
}
}  // namespace
}  // extern "C++"

int ctws_edge_features_block(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype, int64_t nz,
                             int64_t ny, int64_t nx, int64_t cz, int64_t cy, int64_t cx, int ignore_label,
                             const uint64_t* nodes, int64_t n_nodes, const uint64_t* edges, int64_t n_edges,
                             double* out, int64_t* n_missing) {
    return edge_features_block(h, labels, data, data_dtype, nz, ny, nx, cz, cy, cx, ignore_label, nodes, n_nodes,
                               edges, n_edges, out, n_missing, false);
}

int ctws_edge_features_block_device(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype,
                                    int64_t nz, int64_t ny, int64_t nx, int64_t cz, int64_t cy, int64_t cx,
                                    int ignore_label, const uint64_t* nodes, int64_t n_nodes, const uint64_t* edges,
                                    int64_t n_edges, double* out, int64_t* n_missing) {
    return edge_features_block(h, labels, data, data_dtype, nz, ny, nx, cz, cy, cx, ignore_label, nodes, n_nodes,
                               edges, n_edges, out, n_missing, true);
}

// ---- LiftedFeaturesFromNodeLabelsWorkflow: the sparse lifted neighbourhood (k_lifted.hip) ----
extern "C++" {
namespace {
// The first capacity of the key buffer depends on the number of labelled nodes alone: 64 keys per
// source (at depth 4 the 128^3 grid of the benchmark emits 19, a block's RAG 43), and never fewer than 2^16.
constexpr int64_t kLfFirstCap = 1 << 16;
constexpr int64_t kLfCapPerSource = 64;
int64_t lf_first_cap(int64_t ns) { return std::max(kLfFirstCap, kLfCapPerSource * ns); }
// Three workgroups of k_lf_bfs share a CU's LDS (54,272 B each); every wave owns a queue and a
// bitmap over the n nodes (4 1/8 bytes per node), and the waves in flight are cut down to what fits
// in this many bytes and in half of the free memory
constexpr int kLfMaxGroups = 256 * 3;
constexpr size_t kLfWaveBudget = (size_t)32 << 30;
// the counter block: the row checks' three words, the sources, and a line for the append counter
enum LfWord : size_t { kLfWordSources = 16, kLfWordEmit = 32, kLfWordVisits = 33, kLfWords = 48 };

int lifted_neighborhood(ctws_handle* h, const uint64_t* edges, int64_t m, const uint64_t* labels, int64_t n, int depth,
                        int mode, uint64_t ignore_label, uint64_t* out, int64_t cap, int64_t* n_out, bool dev) {
    int r;
    if (!h) return CTWS_EINVAL;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    if (n_out) *n_out = 0;
    if (!n_out || m < 0 || n < 0 || cap < 0 || (!out && cap > 0) || (m > 0 && !edges) || (n > 0 && !labels)) {
        h->err = "lifted neighborhood: bad arguments (tables for n_edges > 0 and n_nodes > 0, out for cap > 0)";
        return CTWS_EINVAL;
    }
    if (depth < 1) {
        h->err = "lifted neighborhood: depth " + std::to_string(depth) + " (a lifted edge spans at least 2 hops; depth >= 1)";
        return CTWS_EINVAL;
    }
    if (mode != CTWS_LIFTED_ALL && mode != CTWS_LIFTED_SAME && mode != CTWS_LIFTED_DIFFERENT) {
        h->err = "lifted neighborhood: unknown mode " + std::to_string(mode) + " (0 all, 1 same, 2 different)";
        return CTWS_EINVAL;
    }
    if (n >= (1ll << 32) || m >= (1ll << 31)) {
        h->err = "lifted neighborhood: 2^32 or more nodes or 2^31 or more edges (ids and adjacency offsets are 32-bit)";
        return CTWS_EUNSUPPORTED;
    }
    if (m == 0) return CTWS_OK;  // no edge, no path: no launch
    if (n == 0) {
        h->err = "lifted neighborhood: " + std::to_string(m) + " rows hold an id >= n_nodes (0)";
        return CTWS_EINVAL;
    }
    const uint64_t *de, *dl;
    if ((r = stage_in(h, h->lf_edges, edges, 2 * sizeof(uint64_t) * (size_t)m, dev, &de)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->lf_lab, labels, sizeof(uint64_t) * (size_t)n, dev, &dl)) != CTWS_OK) return r;
    const size_t nb1 = sizeof(uint32_t) * ((size_t)n + 1);
    if ((r = grow(h, h->lf_red, kLfWords * sizeof(uint64_t))) != CTWS_OK) return r;
    if ((r = grow(h, h->lf_deg, nb1)) != CTWS_OK) return r;
    if ((r = grow(h, h->lf_row, nb1)) != CTWS_OK) return r;
    if ((r = grow(h, h->lf_adj, 2 * sizeof(uint32_t) * (size_t)m)) != CTWS_OK) return r;
    if ((r = grow(h, h->lf_src, sizeof(uint32_t) * (size_t)n)) != CTWS_OK) return r;
    unsigned long long* red = (unsigned long long*)h->lf_red.p;
    uint32_t* deg = (uint32_t*)h->lf_deg.p;
    uint32_t* row = (uint32_t*)h->lf_row.p;
    // the rows' checks with the degrees, and the labelled nodes
    HIPCHK(hipMemsetAsync(red, 0, kLfWords * sizeof(uint64_t), h->stream));
    HIPCHK(hipMemsetAsync(deg, 0, nb1, h->stream));
    record(h, 0);
    const unsigned gm = (unsigned)std::min<int64_t>((m + 255) / 256, 8192);
    const unsigned gn = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    k_lf_degrees<<<gm, 256, 0, h->stream>>>(de, (uint32_t)m, (uint64_t)n, deg, red);
    k_lf_sources<<<gn, 256, 0, h->stream>>>(dl, (uint32_t)n, ignore_label, (uint32_t*)h->lf_src.p, red + kLfWordSources);
    LAUNCHCHK();
    unsigned long long w[kLfWordSources + 1];
    HIPCHK(hipMemcpyAsync(w, red, sizeof(w), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (w[kLfBadId] || w[kLfBadUv] || w[kLfBadOrder]) {
        h->err = "lifted neighborhood: the edge table is not a graph's: " + std::to_string(w[kLfBadId]) +
                 " rows hold an id >= n_nodes (" + std::to_string(n) + "), " + std::to_string(w[kLfBadUv]) +
                 " rows have u >= v, " + std::to_string(w[kLfBadOrder]) + " rows are not above their predecessor";
        return CTWS_EINVAL;
    }
    const int64_t ns = (int64_t)w[kLfWordSources];
    if (ns > n) {
        h->err = "lifted neighborhood: the kernel counted " + std::to_string(ns) + " labelled nodes of " + std::to_string(n);
        return CTWS_EHIP;
    }
    add_timing(h, "lf_sources", (float)ns);
    if (ns == 0) return CTWS_OK;  // no labelled node: no search
    // CSR of both directions
    size_t tb_scan = 0;
    HIPCHK(lf_scan(nullptr, tb_scan, nullptr, nullptr, n + 1, h->stream));
    if ((r = grow(h, h->lf_tmp, tb_scan)) != CTWS_OK) return r;
    HIPCHK(lf_scan(h->lf_tmp.p, tb_scan, deg, row, n + 1, h->stream));
    HIPCHK(hipMemsetAsync(deg, 0, nb1, h->stream));  // (now the fill's cursors)
    k_lf_fill<<<gm, 256, 0, h->stream>>>(de, (uint32_t)m, row, deg, (uint32_t*)h->lf_adj.p);
    LAUNCHCHK();
    record(h, 1);
    // the waves in flight and their queues and bitmaps
    const uint32_t qstride = (uint32_t)std::max<int64_t>(n - kLfQueueLds, 1);
    const uint32_t bstride = (uint32_t)((n + 31) / 32);
    const size_t wave_bytes = sizeof(uint32_t) * ((size_t)qstride + bstride);
    int64_t groups = std::min<int64_t>((ns + kLfWaves - 1) / kLfWaves, kLfMaxGroups);
    size_t free_bytes = 0, total_bytes = 0;
    HIPCHK(hipMemGetInfo(&free_bytes, &total_bytes));
    // (what the handle holds already is its own: a second call takes the waves of the first)
    const size_t budget = std::max(h->lf_queue.bytes + h->lf_bits.bytes, std::min(kLfWaveBudget, free_bytes / 2));
    groups = std::max<int64_t>(1, std::min<int64_t>(groups, (int64_t)(budget / wave_bytes) / kLfWaves));
    const size_t nwaves = (size_t)groups * kLfWaves;
    if ((r = grow(h, h->lf_queue, sizeof(uint32_t) * qstride * nwaves)) != CTWS_OK) return r;
    if ((r = grow(h, h->lf_bits, sizeof(uint32_t) * bstride * nwaves)) != CTWS_OK) return r;
    HIPCHK(hipMemsetAsync(h->lf_bits.p, 0, sizeof(uint32_t) * bstride * nwaves, h->stream));
    int b = 1;  // bits per node id
    while ((1ll << b) < n) ++b;
    LfArgs a;
    a.row = row;
    a.adj = (const uint32_t*)h->lf_adj.p;
    a.lab = dl;
    a.src = (const uint32_t*)h->lf_src.p;
    a.ns = (uint32_t)ns;
    a.depth = (uint32_t)depth;
    a.mode = mode;
    a.ignore = ignore_label;
    a.b = b;
    a.queue = (uint32_t*)h->lf_queue.p;
    a.qstride = qstride;
    a.bits = (uint32_t*)h->lf_bits.p;
    a.bstride = bstride;
    a.count = red + kLfWordEmit;
    a.visits = red + kLfWordVisits;
    EmitCap ecap = {kRedEmit, (unsigned long long)lf_first_cap(ns)};
    Emitted e;
    r = counted_emit(
        h, "lifted neighborhood", red + kLfWordEmit, 2, 2, &ecap, 1,
        [&] {
            const int r = grow(h, h->lf_keys, sizeof(uint64_t) * (size_t)ecap.cap);
            if (r != CTWS_OK) return r;
            a.keys = (uint64_t*)h->lf_keys.p;
            a.cap = ecap.cap;
            k_lf_bfs<<<(unsigned)groups, 64 * kLfWaves, 0, h->stream>>>(a);
            return CTWS_OK;
        },
        [](const unsigned long long*) { return CTWS_OK; }, &e);
    if (r != CTWS_OK) return r;
    record(h, 2);
    const unsigned long long k = e.w[kRedEmit];
    add_timing(h, "lf_bfs_passes", (float)e.passes);
    add_timing(h, "lf_keys", (float)k);
    add_timing(h, "lf_visits", (float)e.w[1]);
    add_timing(h, "lf_waves", (float)nwaves);
    if (k >= (1ull << 31)) {
        h->err = "lifted neighborhood: 2^31 or more lifted edges (" + std::to_string(k) + ") in one call";
        return CTWS_EUNSUPPORTED;
    }
    *n_out = (int64_t)k;
    if ((int64_t)k > cap) {
        h->err = "lifted neighborhood: output capacity too small";
        return CTWS_EINVAL;
    }
    if (k == 0) {
        HIPCHK(hipStreamSynchronize(h->stream));
        return CTWS_OK;
    }
    uint64_t* dout;
    const size_t out_bytes = 2 * sizeof(uint64_t) * (size_t)k;
    if ((r = out_begin(h, h->lf_out, out, out_bytes, dev, &dout)) != CTWS_OK) return r;
    size_t tb_sort = 0;
    HIPCHK(lf_sort(nullptr, tb_sort, nullptr, nullptr, (int64_t)k, 2 * b, h->stream));
    if ((r = grow(h, h->lf_skeys, sizeof(uint64_t) * (size_t)k)) != CTWS_OK) return r;
    if ((r = grow(h, h->lf_tmp, tb_sort)) != CTWS_OK) return r;
    HIPCHK(lf_sort(h->lf_tmp.p, tb_sort, (const uint64_t*)h->lf_keys.p, (uint64_t*)h->lf_skeys.p, (int64_t)k, 2 * b,
                   h->stream));
    const unsigned gk = (unsigned)std::min<int64_t>(((int64_t)k + 255) / 256, 8192);
    k_lf_unpack<<<gk, 256, 0, h->stream>>>((const uint64_t*)h->lf_skeys.p, (int64_t)k, b, dout);
    LAUNCHCHK();
    record(h, 3);
    if ((r = out_end(h, out, dout, out_bytes, dev)) != CTWS_OK) return r;
    stage_time(h, "lf_csr", 0, 1);
    stage_time(h, "lf_bfs", 1, 2);
    stage_time(h, "lf_sort", 2, 3);
    return CTWS_OK;
}
}  // namespace
}  // extern "C++"

int ctws_lifted_neighborhood(ctws_handle* h, const uint64_t* edges, int64_t n_edges, const uint64_t* node_labels,
                             int64_t n_nodes, int depth, int mode, uint64_t ignore_label, uint64_t* out, int64_t cap,
                             int64_t* n_out) {
    return lifted_neighborhood(h, edges, n_edges, node_labels, n_nodes, depth, mode, ignore_label, out, cap, n_out,
                               false);
}

int ctws_lifted_neighborhood_device(ctws_handle* h, const uint64_t* edges, int64_t n_edges,
                                    const uint64_t* node_labels, int64_t n_nodes, int depth, int mode,
                                    uint64_t ignore_label, uint64_t* out, int64_t cap, int64_t* n_out) {
    return lifted_neighborhood(h, edges, n_edges, node_labels, n_nodes, depth, mode, ignore_label, out, cap, n_out,
                               true);
}

int ctws_lifted_limits(int64_t n_sources, int64_t* first_capacity, int64_t* visited_capacity) {
    if (n_sources < 0) return CTWS_EINVAL;
    if (first_capacity) *first_capacity = lf_first_cap(n_sources);
    if (visited_capacity) *visited_capacity = kLfHashFill;
    return CTWS_OK;
}

// ---- ConnectedComponentsWorkflow, SizeFilterAndGraphWatershedWorkflow: graph components and the
// ---- seeded graph watershed over the merged graph's edge table (k_graphpost.hip) ----
extern "C++" {
namespace {
// the counter block: the edge checks' words, and a line for a round's hooks and a pass's open flag
enum GpWord : size_t { kGpWordHooks = 16, kGpWordOpen = 17, kGpWords = 32 };

unsigned gp_grid(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 8192); }

// the checks both calls share; *done: nothing is left to do (no node)
int gp_begin(ctws_handle* h, const char* what, const void* edges, int64_t m, const void* nodes, int64_t n, const void* out,
             bool* done) {
    int r;
    *done = false;
    if ((r = call_begin(h)) != CTWS_OK) return r;
    if (m < 0 || n < 0 || (m > 0 && !edges) || (n > 0 && (!nodes || !out))) {
        h->err = std::string(what) + ": bad arguments (an edge table for n_edges > 0, node arrays for n_nodes > 0)";
        return CTWS_EINVAL;
    }
    if (n >= (1ll << 32) || m >= (1ll << 32)) {
        h->err = std::string(what) + ": 2^32 or more nodes or edges (node ids and edge ranks are 32-bit)";
        return CTWS_EUNSUPPORTED;
    }
    if (n == 0) {
        if (m > 0) {
            h->err = std::string(what) + ": " + std::to_string(m) + " rows hold an id >= n_nodes (0)";
            return CTWS_EINVAL;
        }
        *done = true;
    }
    return CTWS_OK;
}

// the edge checks' counters of a call; the stream has drained when this returns
int gp_edge_check(ctws_handle* h, const char* what, unsigned long long* red, int64_t n) {
    unsigned long long w[2];
    HIPCHK(hipMemcpyAsync(w, red, sizeof(w), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (w[kGpBadId] || w[kGpBadNan]) {
        h->err = std::string(what) + ": " + std::to_string(w[kGpBadId]) + " rows hold an id >= n_nodes (" +
                 std::to_string(n) + "), " + std::to_string(w[kGpBadNan]) + " weights are NaN";
        return CTWS_EINVAL;
    }
    return CTWS_OK;
}

// lab (n, on the device) renumbered in place by first appearance over the index, from 1, zeros kept
int gp_relabel(ctws_handle* h, uint64_t* lab, int64_t n) {
    int r;
    if ((r = grow(h, h->gp_keys, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_skeys, sizeof(uint64_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_idx, sizeof(uint32_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_sidx, sizeof(uint32_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_best, sizeof(uint32_t) * (size_t)n)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_num, sizeof(uint32_t) * (size_t)n)) != CTWS_OK) return r;
    size_t tb_sort = 0, tb_scan = 0;
    HIPCHK(gp_sort(nullptr, tb_sort, nullptr, nullptr, nullptr, nullptr, n, h->stream));
    HIPCHK(gp_scan(nullptr, tb_scan, nullptr, nullptr, n, h->stream));
    if ((r = grow(h, h->gp_tmp, std::max(tb_sort, tb_scan))) != CTWS_OK) return r;
    uint64_t *keys = (uint64_t*)h->gp_keys.p, *skeys = (uint64_t*)h->gp_skeys.p;
    uint32_t *idx = (uint32_t*)h->gp_idx.p, *sidx = (uint32_t*)h->gp_sidx.p;
    uint32_t *flag = (uint32_t*)h->gp_best.p, *num = (uint32_t*)h->gp_num.p;
    const unsigned gn = gp_grid(n);
    k_gp_rl_keys<<<gn, 256, 0, h->stream>>>(lab, (uint64_t)n, keys, idx, flag);
    HIPCHK(gp_sort(h->gp_tmp.p, tb_sort, keys, skeys, idx, sidx, n, h->stream));
    k_gp_rl_heads<<<gn, 256, 0, h->stream>>>(skeys, sidx, (uint64_t)n, flag);
    HIPCHK(gp_scan(h->gp_tmp.p, tb_scan, flag, num, n, h->stream));
    k_gp_rl_write<<<gn, 256, 0, h->stream>>>(skeys, sidx, num, (uint64_t)n, lab);
    LAUNCHCHK();
    return CTWS_OK;
}

int graph_components(ctws_handle* h, const uint64_t* edges, int64_t m, const uint64_t* assignments, int64_t n,
                     uint64_t* out, bool dev) {
    const char* what = "graph components";
    int r;
    bool done;
    if (!h) return CTWS_EINVAL;
    if ((r = gp_begin(h, what, edges, m, assignments, n, out, &done)) != CTWS_OK || done) return r;
    const uint64_t *de = nullptr, *da;
    if (m > 0 && (r = stage_in(h, h->gp_edges, edges, 2 * sizeof(uint64_t) * (size_t)m, dev, &de)) != CTWS_OK) return r;
    if ((r = stage_in(h, h->gp_in, assignments, sizeof(uint64_t) * (size_t)n, dev, &da)) != CTWS_OK) return r;
    const size_t nb = sizeof(uint32_t) * (size_t)n;
    if ((r = grow(h, h->gp_red, kGpWords * sizeof(uint64_t))) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_parent, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_best, nb)) != CTWS_OK) return r;
    if ((r = grow(h, h->gp_num, nb)) != CTWS_OK) return r;
    size_t tb_scan = 0;
    HIPCHK(gp_scan(nullptr, tb_scan, nullptr, nullptr, n, h->stream));
    if ((r = grow(h, h->gp_tmp, tb_scan)) != CTWS_OK) return r;
    unsigned long long* red = (unsigned long long*)h->gp_red.p;
    uint32_t *parent = (uint32_t*)h->gp_parent.p, *flag = (uint32_t*)h->gp_best.p, *num = (uint32_t*)h->gp_num.p;
    const unsigned gn = gp_grid(n);
    record(h, 0);
    k_gp_init<<<gn, 256, 0, h->stream>>>(parent, nullptr, (uint64_t)n);
    if (m > 0) {  // (no edge: no edge kernel, every labelled node is a component)
        HIPCHK(hipMemsetAsync(red, 0, kGpWords * sizeof(uint64_t), h->stream));
        k_gp_union<<<gp_grid(m), 256, 0, h->stream>>>(de, (uint64_t)m, (uint64_t)n, da, parent, red);
        LAUNCHCHK();
        if ((r = gp_edge_check(h, what, red, n)) != CTWS_OK) return r;  // (before anything is written to out)
        k_gp_compress<<<gn, 256, 0, h->stream>>>(parent, (uint64_t)n);
    }
    record(h, 1);
    uint64_t* dout;
    const size_t out_bytes = sizeof(uint64_t) * (size_t)n;
    if ((r = out_begin(h, h->gp_out, out, out_bytes, dev, &dout)) != CTWS_OK) return r;
    k_gp_cc_flag<<<gn, 256, 0, h->stream>>>(parent, da, (uint64_t)n, flag);
    HIPCHK(gp_scan(h->gp_tmp.p, tb_scan, flag, num, n, h->stream));
    k_gp_cc_write<<<gn, 256, 0, h->stream>>>(parent, da, num, (uint64_t)n, dout);
    LAUNCHCHK();
    record(h, 2);
    if ((r = out_end(h, out, dout, out_bytes, dev)) != CTWS_OK) return r;
    stage_time(h, "gc_union", 0, 1);
    stage_time(h, "gc_number", 1, 2);
    return CTWS_OK;
}

int graph_watershed(ctws_handle* h, const uint64_t* edges, const double* weights, int64_t m, const uint64_t* seeds,
                    int64_t n, int relabel, uint64_t* out, bool dev) {
    const char* what = "graph watershed";
    int r;
    bool done;
    if (!h) return CTWS_EINVAL;
    if ((r = gp_begin(h, what, edges, m, seeds, n, out, &done)) != CTWS_OK || done) return r;
    if (m > 0 && !weights) {
        h->err = "graph watershed: bad arguments (a weight per edge for n_edges > 0)";
        return CTWS_EINVAL;
    }
    if ((const void*)out == (const void*)seeds) {
        h->err = "graph watershed: out is the seed array (a node reads its root's seed while others are written)";
        return CTWS_EINVAL;
    }
    const uint64_t *de, *ds;
    const double* dw;
    if ((r = stage_in(h, h->gp_in, seeds, sizeof(uint64_t) * (size_t)n, dev, &ds)) != CTWS_OK) return r;
    uint64_t* dout;
    const size_t out_bytes = sizeof(uint64_t) * (size_t)n;
    if ((r = out_begin(h, h->gp_out, out, out_bytes, dev, &dout)) != CTWS_OK) return r;
    const unsigned gn = gp_grid(n);
    int rounds = 0, passes = 0;
    record(h, 0);
    if (m == 0) {  // no edge: no edge kernel, the seeds are the result
        if (dout != ds) HIPCHK(hipMemcpyAsync(dout, ds, out_bytes, hipMemcpyDeviceToDevice, h->stream));
        record(h, 1);
        record(h, 2);
    } else {
        if ((r = stage_in(h, h->gp_edges, edges, 2 * sizeof(uint64_t) * (size_t)m, dev, &de)) != CTWS_OK) return r;
        if ((r = stage_in(h, h->gp_w, weights, sizeof(double) * (size_t)m, dev, &dw)) != CTWS_OK) return r;
        const size_t nb = sizeof(uint32_t) * (size_t)n, mb = sizeof(uint32_t) * (size_t)m;
        if ((r = grow(h, h->gp_red, kGpWords * sizeof(uint64_t))) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_parent, nb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_next, nb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_best, nb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_su, mb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_sv, mb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_idx, mb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_sidx, mb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_keys, 2 * mb)) != CTWS_OK) return r;
        if ((r = grow(h, h->gp_skeys, 2 * mb)) != CTWS_OK) return r;
        size_t tb_sort = 0;
        HIPCHK(gp_sort(nullptr, tb_sort, nullptr, nullptr, nullptr, nullptr, m, h->stream));
        if ((r = grow(h, h->gp_tmp, tb_sort)) != CTWS_OK) return r;
        unsigned long long* red = (unsigned long long*)h->gp_red.p;
        uint32_t *parent = (uint32_t*)h->gp_parent.p, *next = (uint32_t*)h->gp_next.p, *best = (uint32_t*)h->gp_best.p;
        uint32_t *su = (uint32_t*)h->gp_su.p, *sv = (uint32_t*)h->gp_sv.p;
        const unsigned gm = gp_grid(m);
        // the checks and the ranks: one stable sort of (ordered weight, edge index)
        HIPCHK(hipMemsetAsync(red, 0, kGpWords * sizeof(uint64_t), h->stream));
        k_gp_keys<<<gm, 256, 0, h->stream>>>(de, dw, (uint64_t)m, (uint64_t)n, (uint64_t*)h->gp_keys.p,
                                             (uint32_t*)h->gp_idx.p, red);
        LAUNCHCHK();
        if ((r = gp_edge_check(h, what, red, n)) != CTWS_OK) return r;
        HIPCHK(gp_sort(h->gp_tmp.p, tb_sort, (const uint64_t*)h->gp_keys.p, (uint64_t*)h->gp_skeys.p,
                       (const uint32_t*)h->gp_idx.p, (uint32_t*)h->gp_sidx.p, m, h->stream));
        k_gp_sorted_ends<<<gm, 256, 0, h->stream>>>(de, (const uint32_t*)h->gp_sidx.p, (uint64_t)m, su, sv);
        k_gp_init<<<gn, 256, 0, h->stream>>>(parent, best, (uint64_t)n);
        LAUNCHCHK();
        record(h, 1);
        // the rounds: both loops are capped here, and a cap that is reached is an error
        bool fixed = false;
        unsigned long long w[2];
        for (int round = 0; round < kGpMaxIters && !fixed; ++round) {
            HIPCHK(hipMemsetAsync(red + kGpWordHooks, 0, 2 * sizeof(uint64_t), h->stream));
            k_gp_offer<<<gm, 256, 0, h->stream>>>(su, sv, (uint64_t)m, parent, ds, best);
            k_gp_hook<<<gn, 256, 0, h->stream>>>(su, sv, parent, ds, best, next, (uint64_t)n, red + kGpWordHooks);
            k_gp_jump<<<gn, 256, 0, h->stream>>>(next, best, (uint64_t)n, red + kGpWordOpen);
            LAUNCHCHK();
            HIPCHK(hipMemcpyAsync(w, red + kGpWordHooks, sizeof(w), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            if (w[0] == 0ull) {  // no component hooked: next is parent, the forest is final
                fixed = true;
                break;
            }
            ++rounds;
            int p = 1;
            for (; w[1] != 0ull && p < kGpMaxIters; ++p) {
                HIPCHK(hipMemsetAsync(red + kGpWordOpen, 0, sizeof(uint64_t), h->stream));
                k_gp_jump<<<gn, 256, 0, h->stream>>>(next, nullptr, (uint64_t)n, red + kGpWordOpen);
                LAUNCHCHK();
                HIPCHK(hipMemcpyAsync(w + 1, red + kGpWordOpen, sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
                HIPCHK(hipStreamSynchronize(h->stream));
            }
            passes += p;
            if (w[1] != 0ull) {
                h->err = "graph watershed: pointer jumping did not reach a fixpoint in " + std::to_string(kGpMaxIters) +
                         " passes (round " + std::to_string(round) + ")";
                return CTWS_EHIP;
            }
            std::swap(parent, next);
        }
        if (!fixed) {
            h->err = "graph watershed: components still hooked after " + std::to_string(kGpMaxIters) + " rounds";
            return CTWS_EHIP;
        }
        record(h, 2);
        k_gp_ws_write<<<gn, 256, 0, h->stream>>>(parent, ds, (uint64_t)n, dout);
        LAUNCHCHK();
    }
    if (relabel && (r = gp_relabel(h, dout, n)) != CTWS_OK) return r;
    record(h, 3);
    if ((r = out_end(h, out, dout, out_bytes, dev)) != CTWS_OK) return r;
    stage_time(h, "gw_sort", 0, 1);
    stage_time(h, "gw_rounds_ms", 1, 2);
    stage_time(h, "gw_write", 2, 3);
    add_timing(h, "gw_rounds", (float)rounds);
    add_timing(h, "gw_jump_passes", (float)passes);
    return CTWS_OK;
}
}  // namespace
}  // extern "C++"

int ctws_graph_components(ctws_handle* h, const uint64_t* edges, int64_t n_edges, const uint64_t* assignments,
                          int64_t n_nodes, uint64_t* out) {
    return graph_components(h, edges, n_edges, assignments, n_nodes, out, false);
}

int ctws_graph_components_device(ctws_handle* h, const uint64_t* edges, int64_t n_edges, const uint64_t* assignments,
                                 int64_t n_nodes, uint64_t* out) {
    return graph_components(h, edges, n_edges, assignments, n_nodes, out, true);
}

int ctws_graph_watershed(ctws_handle* h, const uint64_t* edges, const double* weights, int64_t n_edges,
                         const uint64_t* seeds, int64_t n_nodes, int relabel, uint64_t* out) {
    return graph_watershed(h, edges, weights, n_edges, seeds, n_nodes, relabel, out, false);
}

int ctws_graph_watershed_device(ctws_handle* h, const uint64_t* edges, const double* weights, int64_t n_edges,
                                const uint64_t* seeds, int64_t n_nodes, int relabel, uint64_t* out) {
    return graph_watershed(h, edges, weights, n_edges, seeds, n_nodes, relabel, out, true);
}

// ---- ThresholdedComponentsWorkflow: BlockComponents (k_threshcc.hip) -----------------------
extern "C++" {
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
}  // extern "C++"

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
