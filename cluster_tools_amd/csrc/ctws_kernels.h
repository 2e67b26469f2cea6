// ctws_kernels.h — declarations of the gfx950 kernels (defined in k_*.hip).
#pragma once

#include "ctws_dev.h"

namespace ctws {

struct PrepParams {
    float threshold;
    int invert;
    int agg;
    int px2;
};
struct EdtColParams {
    int axis;
    int p2;
    int final_pass;
    int per_slice;
    uint32_t max_dist;
    int px2;  // x pitch squared: the record-fed y pass computes the x pass's g2 itself
};
struct EdtRealParams {
    double pitch[3];
    int per_slice;  // 2-D dt: per-slice lines (y, x), dmax = Y^2 + X^2
    int real;       // 1: non-integer pitch (double temporary, maxDist = dmax); 0: float, ceil(dmax)
};
struct HmapParams {
    float a, b;
    int per_slice;
};
struct GaussParams {
    int axis;
    int r;
    int hmap_src;
};
struct FilterParams {
    uint32_t size_filter;
    int tz, ty, tx;  // flood tile extents: tiles holding a freed voxel are activated in act
    uint32_t* act;
};

// k_edt.hip
__global__ void k_input_minmax(const BlockDesc*, BlockStat*);
__global__ void k_prep_edt_x(const BlockDesc*, BlockStat*, PrepParams, float*, uint32_t*);
template <int KMAX>
__global__ void k_prep_edt_x_reg(const BlockDesc*, BlockStat*, PrepParams, float*, uint32_t*);
template <int KMAX, class T, bool BITS>
__global__ void k_prep_edt_x_co(const BlockDesc*, BlockStat*, PrepParams, float*, uint32_t*, EdtRec*);
template <class T>
__global__ void k_input_minmax_t(const BlockDesc*, BlockStat*);
constexpr int kEdtSearchCap = 48;  // bounded-search steps before a column goes to k_edt_col_fh
template <int W>
__global__ void k_edt_col(const BlockDesc*, BlockStat*, EdtColParams, const uint32_t*, uint32_t*, float*, uint32_t*,
                          uint32_t*, unsigned long long*, uint32_t*);
__global__ void k_sqrt_int_check(uint32_t, uint32_t, float*);
template <int W, int RING>
__global__ void k_edt_col_bits(const BlockDesc*, BlockStat*, EdtColParams, const EdtRec*, uint32_t*, float*, uint32_t*,
                               uint32_t*, unsigned long long*, uint32_t*);
__global__ void k_edt_col_fh(const BlockDesc*, BlockStat*, EdtColParams, const uint32_t*, const EdtRec*, uint32_t*,
                             float*, uint32_t*, uint32_t*, const unsigned long long*, const uint32_t*);
template <class T>
__global__ void k_edt_real_init(const BlockDesc*, const BlockStat*, EdtRealParams, const uint32_t*, T*);
template <class T>
__global__ void k_edt_real_line(const BlockDesc*, const BlockStat*, int, EdtRealParams, int, T*, char*, int);
template <class T>
__global__ void k_edt_real_final(const BlockDesc*, BlockStat*, EdtRealParams, const T*, float*, uint32_t*, uint32_t*);
__global__ void k_dt_slice_stats(const BlockDesc*, const BlockStat*, const float*, uint32_t*, uint32_t*);
__global__ void k_set_active(const BlockDesc*, BlockStat*, int);

// k_gauss.hip
__global__ void k_hmap(const BlockDesc*, const BlockStat*, HmapParams, const float*, const float*, const uint32_t*,
                       const uint32_t*, float*);
template <int W>
__global__ void k_gauss_col(const BlockDesc*, const BlockStat*, GaussParams, HmapParams, const double*, const float*,
                            const float*, const uint32_t*, const uint32_t*, float*);
__global__ void k_gauss_row(const BlockDesc*, const BlockStat*, GaussParams, HmapParams, const double*, const float*,
                            const float*, const uint32_t*, const uint32_t*, float*);
constexpr int kTapSlot = 4096;  // doubles per taps slot: radius <= 2047
constexpr int kGaussMaxR = 12;  // sliding-window kernels for radius <= 12 (sigma < 4)
template <int W, int R>
__global__ void k_gauss_col_r(const BlockDesc*, const BlockStat*, GaussParams, HmapParams, const double*, const float*,
                              const float*, const uint32_t*, const uint32_t*, float*);
template <int R>
__global__ void k_gauss_row_r(const BlockDesc*, const BlockStat*, GaussParams, HmapParams, const double*, const float*,
                              const float*, const uint32_t*, const uint32_t*, float*);
// fused y + x passes on 2-D tiles: kGaussYxTY rows x (128 - 2R) columns per workgroup (the x pass
// maps 8 threads to each of the 32 rows)
constexpr int kGaussYxTY = 32;
template <int R>
__global__ void k_gauss_yx(const BlockDesc*, const BlockStat*, int, HmapParams, const double*, const double*,
                           const float*, const float*, const uint32_t*, const uint32_t*, float*);

// k_cc.hip
__global__ void k_localmax(const BlockDesc*, BlockStat*, const float*, uint8_t*, const uint32_t*, uint32_t*, uint64_t*,
                           uint64_t*, uint32_t*);
__global__ void k_plateau_flag(const BlockDesc*, const BlockStat*, uint8_t*, uint32_t*);
__global__ void k_plateau_flag_eq(const BlockDesc*, const BlockStat*, uint8_t*, uint32_t*, const uint64_t*);
template <int ND>
__global__ void k_seed_members_eq(const BlockDesc*, BlockStat*, const uint8_t*, const uint32_t*, uint32_t*, uint64_t*,
                                  const uint64_t*, uint32_t*);
__global__ void k_flatten_tile_roots(const BlockDesc*, const BlockStat*, uint32_t*, const uint64_t*, uint64_t*);
__global__ void k_flatten_seeds(const BlockDesc*, const BlockStat*, uint32_t*, const uint64_t*, uint64_t*);
template <int ND>
__global__ void k_seed_members(const BlockDesc*, BlockStat*, const uint8_t*, const uint32_t*, uint32_t*, uint64_t*,
                               uint32_t*);
__global__ void k_seed_union2(const BlockDesc*, const BlockStat*, const uint8_t*, const uint32_t*, const uint32_t*,
                              uint32_t*);

// k_plateau.hip: the flood across a masked block's plateau (entries + min-plus run scans)
__global__ void k_plat_mark(const BlockDesc*, const BlockStat*, const float*, const uint32_t*, uint64_t*, uint64_t*);
template <int ND>
__global__ void k_plat_entry(const BlockDesc*, const BlockStat*, const float*, uint64_t*, const uint64_t*,
                             const uint32_t*);
__global__ void k_plat_scan_x(const BlockDesc*, const BlockStat*, uint64_t*, const uint64_t*, const uint32_t*);
template <int AX>
__global__ void k_plat_scan_col(const BlockDesc*, const BlockStat*, uint64_t*, const uint64_t*, const uint32_t*);
__global__ void k_plat_restore(const BlockDesc*, const BlockStat*, uint64_t*, const uint64_t*, uint64_t*);
__global__ void k_bitmap_csum(const BlockDesc*, const BlockStat*, int, const uint64_t*, uint32_t*);
__global__ void k_chunk_scan(const BlockDesc*, BlockStat*, int, uint32_t*, int);
__global__ void k_word_prefix(const BlockDesc*, const BlockStat*, int, const uint64_t*, const uint32_t*, uint32_t*);
__global__ void k_root_label(const BlockDesc*, const BlockStat*, int, uint32_t*, const uint64_t*, const uint32_t*,
                             uint32_t*);
__global__ void k_seed_label(const BlockDesc*, const BlockStat*, const uint32_t*, const uint64_t*, const float*,
                             uint32_t*, uint64_t*, uint8_t*, int);
__global__ void k_output(const BlockDesc*, BlockStat*, const uint32_t*, const uint64_t*, int, const uint32_t*,
                         const uint32_t*, const uint32_t*, unsigned long long*, int);
__global__ void k_count_ids(const BlockDesc*, BlockStat*, const uint64_t*);

// k_tilecc.hip: LDS block-based union-find (plateaus, seed CC, halo-crop CC)
enum CcMode { CC_PLATEAU = 0, CC_SEED = 1, CC_CROP = 2 };
struct CcArgs {
    const float* v;        // PLATEAU: seed map
    const uint8_t* cls;    // PLATEAU / SEED: local-max classes (k_localmax)
    const uint32_t* Pp;    // SEED: plateau parents (is_max)
    const uint32_t* lab;   // CROP: flood labels (non-packed)
    const uint64_t* key;   // CROP: packed keys
    int packed;            // CROP
    uint64_t* troot;       // CROP: tile-root bitmap (inner C index, per block at fbase), zeroed;
                           // SEED: the members (seed voxels; outer rows), zeroed.  The seed forest's
                           // parents are written for members only: readers test this bitmap first
    uint64_t* xface;       // CROP: per tile, its low and high x columns as (root << 32 | label)
                           // (k_tile_cc writes, k_tile_merge's x face reads; per block at xcbase)
    const uint32_t* ptile; // PLATEAU: per tile, nonzero if it holds a plateau voxel (k_localmax;
                           // per block at ptbase)
};
template <int ND>
struct CcTile;
template <>
struct CcTile<3> {
    static constexpr int TZ = 4, TY = 16, TX = 32;
};
template <>
struct CcTile<2> {
    static constexpr int TZ = 1, TY = 32, TX = 64;
};
// the tile of one CC mode: 3-D plateau / seed CC in 8-deep tiles (half the z faces of
// k_tile_merge: config 4's seeds stage 11.98 -> 11.29 ms); the crop CC keeps 4-deep tiles
// (its k_tile_cc at 8 deep: 5.6 -> 7.7 ms per step, more than the merge saves)
template <int ND, int MODE>
struct CcTileM : CcTile<ND> {};
template <>
struct CcTileM<3, CC_PLATEAU> {
    static constexpr int TZ = 8, TY = 16, TX = 32;
};
template <>
struct CcTileM<3, CC_SEED> : CcTileM<3, CC_PLATEAU> {};
template <int ND, int MODE>
__global__ void k_tile_cc(const BlockDesc*, const BlockStat*, CcArgs, uint32_t*);
template <int ND>
__global__ void k_output_crop(const BlockDesc*, BlockStat*, const uint32_t*, const uint64_t*);
template <int ND, int MODE>
__global__ void k_tile_merge(const BlockDesc*, const BlockStat*, CcArgs, uint32_t*);

// k_flood.hip
template <int ND>
__global__ void k_flood(const BlockDesc*, const BlockStat*, const float*, uint64_t*, uint32_t*, const uint32_t*,
                        uint32_t*, uint32_t*);

template <int ND>
__global__ void k_flood_packed(const BlockDesc*, const BlockStat*, const float*, uint64_t*, const uint8_t*,
                               const uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*);
constexpr int kLineWords = 24;
constexpr int kStatSlots = 64;  // flood statistics: counter[4 + slot * 4 + k]  // per tile: 8 words of line bits for each of x, y, z
__global__ void k_unpack_labels(const BlockDesc*, const BlockStat*, const uint64_t*, uint32_t*);
template <int ND>
__global__ void k_descent_tile(const BlockDesc*, const BlockStat*, const float*, const uint32_t*, const uint32_t*,
                               const uint64_t*, uint32_t*);
template <int U>
__global__ void k_descent_init(const BlockDesc*, const BlockStat*, const float*, const uint32_t*, uint64_t*, uint8_t*,
                               uint64_t*, uint64_t*, uint32_t*, uint32_t*);
template <int ND, int CW, int CY, int CZ>
__global__ void k_frontier(const BlockDesc*, const BlockStat*, const float*, uint64_t*, const uint64_t*,
                           const uint64_t*, uint64_t*, const uint32_t*, uint32_t*, int, const uint32_t*,
                           const uint32_t*, uint32_t*, uint32_t*, uint32_t*, uint32_t*, int, int);
// k_eval.hip (VI / Rand contingency table)
__global__ void k_eval_add(const uint64_t*, const uint64_t*, int64_t, int, uint64_t*, unsigned long long*, int64_t,
                           uint64_t*, unsigned long long*, int64_t, uint64_t*, unsigned long long*, int64_t,
                           unsigned long long*);
__global__ void k_eval_reduce(const uint64_t*, const unsigned long long*, int64_t, const uint64_t*,
                              const unsigned long long*, int64_t, const uint64_t*, const unsigned long long*, int64_t,
                              const unsigned long long*, double*);
// k_seeded.hip (WatershedFromSeeds)
__global__ void k_fs_active(const BlockDesc*, BlockStat*, int);
// (V: uint32_t = WatershedFromSeeds' uint32 cast, uint64_t = the filling size filter's full ids)
template <class V>
__global__ void k_fs_insert(const BlockDesc*, BlockStat*, uint64_t*);
template <class V>
__global__ void k_fs_collect(const BlockDesc*, BlockStat*, const uint64_t*, V*);
__global__ void k_fs_offsets(const BlockDesc*, const BlockStat*, int, int*, int*);
template <class V>
__global__ void k_fs_rank(const BlockDesc*, const BlockStat*, const uint64_t*, const V*, uint32_t*);
template <class V>
__global__ void k_fs_label(const BlockDesc*, const BlockStat*, const uint64_t*, const uint32_t*, const float*, uint32_t*,
                           uint64_t*, uint8_t*, int);
__global__ void k_fs_auto_label(const BlockDesc*, BlockStat*, const uint32_t*, const uint64_t*, const uint32_t*,
                                const float*, uint32_t*, uint64_t*, uint8_t*, int);
template <class V>
__global__ void k_fs_output(const BlockDesc*, BlockStat*, const uint32_t*, const uint64_t*, int, const V*,
                            const uint32_t*, int);
hipError_t fs_segmented_sort(void* tmp, size_t& bytes, const uint32_t* in, uint32_t* out, int n, int nseg,
                             const int* beg, const int* end, hipStream_t stream);
hipError_t fs_segmented_sort(void* tmp, size_t& bytes, const uint64_t* in, uint64_t* out, int n, int nseg,
                             const int* beg, const int* end, hipStream_t stream);
// k_sizefilter.hip (postprocess SizeFilterWorkflow: membership in the discard set, raw height map)
struct SfDiscard {
    const uint64_t* ids;   // the discard ids, ascending
    int64_t n;
    const uint64_t* bits;  // a bitmap over [lo, hi] (bit id - lo) when the range is small, else nullptr
    uint64_t lo, hi;       // ids[0], ids[n - 1]; an empty set has lo > hi
};
struct SfBlock {
    const uint64_t* lab;  // the block's labels
    uint64_t* seeds;      // out: the labels, 0 where discarded
    int64_t N;
};
__global__ void k_sf_member(const SfBlock*, BlockStat*, SfDiscard);
__global__ void k_sf_hmap(const BlockDesc*, float*);
// per-chunk arrays (generations, queued marks) are indexed at fbase >> kChunkShift: a block's
// frontier words hold at least 2^kChunkShift words per chunk (every brick is 64 words)
constexpr int kChunkShift = 6;
template <int CW, int CY, int CZ>
__global__ void k_frontier_list0(const BlockDesc*, const BlockStat*, const uint64_t*, uint32_t*, uint32_t*);
__global__ void k_frontier_tiles(const BlockDesc*, const BlockStat*, const uint64_t*, uint32_t*, int, int, int);
template <int ND>
__global__ void k_flood_verify(const BlockDesc*, const BlockStat*, const float*, const uint64_t*, const uint64_t*,
                               uint32_t*);
constexpr int kHist2dBins = 8192;  // LDS bins of the per-slice histograms (k_hist2d, k_flood_verify_hist2d)
constexpr int kVerifyHistThreads = 256;  // workgroup of k_flood_verify_hist2d
__global__ void k_flood_verify_hist2d(const BlockDesc*, const BlockStat*, const float*, const uint64_t*,
                                      const uint64_t*, const uint32_t*, uint32_t*, uint32_t*, int, int);
constexpr int kWordWaves = 4;  // waves per workgroup of the word-tiled kernels
__global__ void k_flood_reset(const BlockDesc*, const BlockStat*, const float*, const uint32_t*, const uint32_t*,
                              const uint64_t*, uint64_t*, uint8_t*);

// k_post.hip
__global__ void k_slice_seed_base(const BlockDesc*, const BlockStat*, const uint64_t*, const uint32_t*, uint32_t*);
__global__ void k_hist_zero(const BlockDesc*, const BlockStat*, uint32_t*);
template <int PACKED>
__global__ void k_hist(const BlockDesc*, const BlockStat*, const uint32_t*, const uint64_t*, uint32_t*, int);
constexpr int kHistBins = 16384;  // largest LDS histogram of k_hist
__global__ void k_size_filter(const BlockDesc*, const BlockStat*, FilterParams, const uint32_t*, const uint8_t*,
                              const float*, uint32_t*, uint64_t*, uint8_t*, uint32_t*, int);
__global__ void k_slice_max(const BlockDesc*, const BlockStat*, const uint32_t*, const uint64_t*, int, const uint32_t*,
                            uint32_t*, int, int);
template <int PACKED>
__global__ void k_hist2d(const BlockDesc*, const BlockStat*, const uint32_t*, const uint64_t*, const uint32_t*,
                         uint32_t*, int);
constexpr int kSfPlanSplit = 32;      // workgroups per block of k_sf_plan, at the most
constexpr int kSfPlanLabels = 4096;   // labels per workgroup of k_sf_plan
__global__ void k_sf_plan(const BlockDesc*, BlockStat*, uint32_t, const uint32_t*, const uint8_t*, const uint32_t*,
                          uint32_t*, uint32_t*);
__global__ void k_sf_sparse(const BlockDesc*, BlockStat*, uint32_t, const uint32_t*, const uint8_t*,
                            const uint32_t*, const float*, uint64_t*, uint8_t*, uint64_t*, uint64_t*);
__global__ void k_fixed_from_open(const BlockDesc*, const BlockStat*, const uint64_t*, uint8_t*);
template <int U>
__global__ void k_regrow_init(const BlockDesc*, const BlockStat*, uint32_t, const uint32_t*, const uint8_t*,
                              const float*, uint64_t*, uint8_t*, uint64_t*, uint64_t*, uint32_t*);
__global__ void k_auto_minima(const BlockDesc*, const BlockStat*, const float*, const uint32_t*, uint64_t*);
__global__ void k_auto_seed_set(const BlockDesc*, BlockStat*, const float*, const uint32_t*, const uint64_t*,
                                const uint32_t*, const uint32_t*, uint64_t*, uint8_t*, uint64_t*, uint64_t*, uint32_t*);
__global__ void k_slice_offsets(const BlockDesc*, const BlockStat*, const uint32_t*, uint32_t*);
__global__ void k_finalize_ws(const BlockDesc*, const BlockStat*, const uint32_t*, const uint32_t*, const uint64_t*, int,
                              uint32_t*);

// k_pass2.hip (two-pass watershed, pass 2)
__global__ void k_p2_zero_dt(const BlockDesc*, const BlockStat*, float*);
__global__ void k_p2_insert(const BlockDesc*, BlockStat*, uint64_t*, uint32_t*, const uint32_t*, const uint64_t*,
                            const uint32_t*, const uint32_t*);
__global__ void k_p2_roots(const BlockDesc*, const BlockStat*, const uint64_t*, const uint32_t*, uint64_t*);
__global__ void k_p2_label(const BlockDesc*, const BlockStat*, const uint64_t*, const uint32_t*, const uint64_t*,
                           const uint32_t*, const float*, uint32_t*, uint64_t*, uint8_t*, uint32_t*, uint32_t*, int, int,
                           const uint32_t*, const uint64_t*, const uint32_t*, const uint32_t*, uint8_t*);
__global__ void k_p2_excl_zero(const BlockDesc*, const BlockStat*, uint8_t*);
__global__ void k_p2_excl(const BlockDesc*, const BlockStat*, const uint32_t*, uint8_t*);
__global__ void k_p2_check(const BlockDesc*, BlockStat*, const uint64_t*, const uint32_t*);
__global__ void k_p2_output(const BlockDesc*, BlockStat*, const uint32_t*, const uint64_t*, int, const uint32_t*,
                            const uint32_t*, const uint32_t*);
__global__ void k_slice_inmask(const BlockDesc*, const BlockStat*, uint32_t*);

// k_relabel.hip (RelabelWorkflow: sorted uniques, assignment-table lookup)
__global__ void k_copy_to_host(const uint4*, uint4*, size_t);
__global__ void k_u64_range(const uint64_t*, int64_t, unsigned long long*);
__global__ void k_u64_bits(const uint64_t*, int64_t, uint64_t, unsigned long long*);
__global__ void k_bits_chunk_count(const uint64_t*, int64_t, uint32_t*);
__global__ void k_scan_chunks(const uint32_t*, int64_t, uint64_t*);
__global__ void k_bits_compact(const uint64_t*, int64_t, const uint64_t*, uint64_t, uint64_t, uint64_t*);
__global__ void k_u64_lookup(uint64_t*, int64_t, const uint64_t*, const uint64_t*, int64_t, unsigned long long*);
// k_rag.hip (GraphWorkflow: face-adjacent id pairs of a block, sorted unique pairs with summed weights)
struct RagArgs {
    const uint64_t* lab;        // the block's labels, (nz, ny, nx)
    uint32_t nz, ny, nx;        // nz * ny * nx < 2^31
    int ignore;                 // ignore_label: pairs with a 0 are dropped
    uint64_t* pairs;            // out: (min, max) per emit, cap x 2
    uint64_t* weights;          // out: the emit's run length
    unsigned long long cap;     // emits at positions >= cap are counted, not written
    unsigned long long* count;  // the append counter
    uint64_t* nodes;            // out: the ids of the voxels whose three upper neighbours differ
    unsigned long long ncap;    // as cap, for nodes
    unsigned long long* ncount;
};
__global__ void k_rag_pairs(RagArgs);
__global__ void k_pair_keys(const uint64_t*, int64_t, const uint64_t*, int64_t, int, uint64_t*, unsigned long long*);
__global__ void k_pair_ones(uint64_t*, int64_t);
__global__ void k_pair_unpack(const uint64_t*, int64_t, const uint64_t*, int, uint64_t*);
// k_overlaps.hip (NodeLabelWorkflow: the (node, label) pairs of two label arrays, as weighted run heads)
struct OvArgs {
    const uint64_t* nodes;      // the fragments, n voxels
    const uint64_t* labels;     // the second label array, n voxels
    uint32_t n;                 // n < 2^31
    int with_ignore;            // voxels with labels[i] == ignore_label are not counted
    uint64_t ignore_label;
    uint64_t* pairs;            // out: (node, label) per emit, cap x 2
    uint64_t* weights;          // out: the emit's run length
    unsigned long long cap;     // emits at positions >= cap are counted, not written
    unsigned long long* count;  // the append counter
};
__global__ void k_ov_pairs(OvArgs);
__global__ void k_ov_rows(const uint64_t*, const uint64_t*, int64_t, uint64_t*);
// k_morph.hip (MorphologyWorkflow: the runs of equal ids along x, then one table row per id)
struct MorphArgs {
    const uint64_t* lab;        // the block's labels, (nz, ny, nx)
    uint32_t nz, ny, nx;        // every extent < 2^19, nz * ny * nx < 2^31
    uint64_t* ids;              // out: the run's id per emit
    uint64_t* recs;             // out: z << 44 | y << 25 | x0 << 6 | (len - 1) per emit
    unsigned long long cap;     // emits at positions >= cap are counted, not written
    unsigned long long* count;  // the append counter
    unsigned long long* vmax;   // the largest id of the block (atomicMax; zeroed)
};
struct MorphBegin {
    uint64_t z, y, x;  // the block's begin: begin + extent <= 2^21 per axis
};
__global__ void k_morph_runs(MorphArgs);
// sorted records per chunk of k_morph_rows: an id's segment that holds whole aligned chunks is split
// over one wave per chunk (measured: DESIGN.md section 3.7)
constexpr int kMorphChunk = 2048;
__global__ void k_morph_rows(const uint64_t*, const uint64_t*, uint32_t, const uint64_t*, const uint64_t*, uint32_t,
                             MorphBegin, unsigned long long*, double*);
__global__ void k_morph_long_rows(const uint64_t*, uint32_t, MorphBegin, const unsigned long long*, double*);
// k_regfeat.hip (RegionFeaturesWorkflow: the runs of equal ids along x with the sum of their values,
// placed by a scan of the rows' run counts, then one [id, n, mean] row per id)
struct RegfeatArgs {
    const uint64_t* lab;        // the block's labels, rows x nx
    const void* data;           // the input map on the same box (the kernel's template type)
    uint32_t rows, nx;          // rows = nz * ny, rows * nx < 2^31
    int with_ignore;            // runs of ignore get length 0 and sum 0
    uint64_t ignore;
    const uint32_t* row_first;  // the exclusive scan of k_regfeat_count's row counts
    uint32_t n;                 // the number of records: the scan's total
    uint64_t* ids;              // out: the run's id per record
    uint64_t* vals;             // out: run length << 32 | record index
    double* sums;               // out: the float64 sum of the run's float32 values
    unsigned long long* vmax;   // the largest id of the block (atomicMax; zeroed)
};
__global__ void k_regfeat_count(const uint64_t*, uint32_t, uint32_t, uint32_t*);
template <class T>
__global__ void k_regfeat_runs(RegfeatArgs);
// sorted records per chunk: an id's segment that holds whole aligned chunks gives them to one wave
// each (k_regfeat_chunks), as k_morph_rows does
constexpr int kRegfeatChunk = kMorphChunk;
__global__ void k_regfeat_chunks(const uint64_t*, const uint64_t*, const double*, uint32_t, uint64_t*, double*);
__global__ void k_regfeat_rows(const uint64_t*, const uint64_t*, const double*, uint32_t, const uint64_t*,
                               const uint64_t*, uint32_t, const uint64_t*, const double*, double*);
// k_regcenter.hip (RegionCentersWorkflow: per object the first voxel of its box with the largest
// exact squared distance to the box's background)
constexpr uint32_t kRcInf = 0xFFFFFFFFu;  // a line without background (every finite value is below 2^31)
// k_rc_small: two uint32 arrays of the box in LDS, 80,000 B, so that two workgroups of 512 threads
// with their reduction words share a CU's 160 KiB (163,840 B)
constexpr int kRcSmallVox = 10000;
constexpr int kRcSmallThreads = 512;
// k_rc_col: the staged tile (line x W) in words, 32,640 B: five workgroups per CU with their
// reduction words
constexpr int kRcColWords = 8160;
struct RcObj {
    uint64_t id;          // the object's voxels: label == id, on all 64 bits
    int64_t off;          // of the box's first voxel in the label buffer, in elements
    int64_t pz, py;       // the z and y pitches in elements (x is contiguous)
    uint32_t nz, ny, nx;  // the box: nz * ny * nx < 2^31
    uint32_t wy, wz;      // k_rc_col's tile width of the y and z pass (0: the line does not fit the LDS)
    uint64_t sbase;       // larger boxes: of the box in the two scratch arrays, in elements
};
struct RcRes {
    uint32_t z2, y2, x2;  // the squared resolutions
};
__global__ void k_rc_small(const uint64_t*, const RcObj*, const uint32_t*, RcRes, unsigned long long*);
__global__ void k_rc_rows(const uint64_t*, const RcObj*, const uint32_t*, RcRes, uint32_t*);
template <bool STAGE>
__global__ void k_rc_col(const RcObj*, const uint32_t*, int, uint32_t, int, const uint32_t*, uint32_t*,
                         unsigned long long*);
__global__ void k_rc_finish(const RcObj*, uint32_t, const unsigned long long*, long long*, uint8_t*);
// k_downscale.hip (DownscalingWorkflow: mean / max / min over fz x fy x fx cells, zero-padded ends)
constexpr int kDsMean = 0, kDsMax = 1, kDsMin = 2;
struct DownscaleArgs {
    const void* in;          // the block (nz, ny, nx) of the kernel's template type
    void* out;               // (oz, oy, ox) = ceil(n / f) per axis, same type
    uint32_t nz, ny, nx;     // nz * ny * nx < 2^31
    uint32_t oz, oy, ox;
    uint32_t fz, fy, fx;     // 1..8 each (k_downscale_vec: FZ, 2, 2)
    uint32_t groups, per;    // k_downscale_vec: 16-byte output groups per row, work items per row
    uint32_t items;          // the work items of the launch
    uint32_t* flag;          // the flag table (zeroed by the caller): a slot |= 1 when a voxel is nonzero
};
// the any-nonzero flag is kDsFlagSlots words, kDsFlagStride words (a cache line) apart, a slot per
// workgroup index modulo kDsFlagSlots: the block holds a nonzero voxel when any slot is set
constexpr int kDsFlagSlots = 128, kDsFlagStride = 32;
template <class T, int FUNC>
__global__ void k_downscale_cell(DownscaleArgs);
template <class T, int FUNC, int FZ>
__global__ void k_downscale_vec(DownscaleArgs);
// k_edgefeat.hip (EdgeFeaturesWorkflow: the boundary-map statistics of a block's edges)
struct EfArgs {
    const uint64_t* lab;          // the block's labels, (nz, ny, nx): the extended box
    const void* data;             // the boundary map on the same box, float32 or uint8
    uint32_t nz, ny, nx;          // nz * ny * nx < 2^31
    uint32_t cz, cy, cx;          // the core extent: a pair belongs to the block of its lower voxel
    int ignore;                   // ignore_label: pairs with a 0 are dropped
    const uint64_t* tab;          // the sub-graph's nodes, ascending
    uint32_t nt;
    int b;                        // bits per rank
    const uint64_t* ekeys;        // the sub-graph's edges as rank(u) << b | rank(v), ascending
    uint32_t ne;
    uint64_t* keys;               // out: edge << 32 | ordered(value), two per owned pair
    unsigned long long cap;       // keys at positions >= cap are counted, not written
    unsigned long long* count;    // the append counter
    unsigned long long* missing;  // owned pairs whose edge is not in the table
};
__global__ void k_ef_edge_keys(const uint64_t*, int64_t, const uint64_t*, int64_t, int, uint64_t*, unsigned long long*);
template <class T>
__global__ void k_ef_samples(EfArgs);
__global__ void k_ef_stats(const uint64_t*, uint32_t, uint32_t, double*);
// k_lifted.hip (LiftedFeaturesFromNodeLabelsWorkflow: the sparse lifted neighbourhood of a graph)
constexpr int kLfWaves = 4;          // waves (= sources in flight) per workgroup of k_lf_bfs
constexpr int kLfHashBits = 11;
constexpr int kLfHashSlots = 1 << kLfHashBits;  // words of a wave's visited hash set in LDS
constexpr int kLfHashFill = 1536;    // nodes a wave's hash set takes before the wave moves to its bitmap
constexpr int kLfProbe = 32;         // slots an insertion looks at before it gives up (then the bitmap)
constexpr int kLfQueueLds = 1024;    // entries of a wave's node list in LDS; the rest in its global queue
constexpr int kLfStage = 128;        // staged keys per wave (a step emits at most 64)
constexpr int kLfModeAll = 0, kLfModeSame = 1, kLfModeDifferent = 2;
// the words of k_lf_degrees' counter block
constexpr int kLfBadId = 0, kLfBadUv = 1, kLfBadOrder = 2;
struct LfArgs {
    const uint32_t* row;        // CSR of both directions: the list of node i is adj[row[i] .. row[i + 1])
    const uint32_t* adj;
    const uint64_t* lab;        // the node labels, (n)
    const uint32_t* src;        // the labelled nodes
    uint32_t ns;
    uint32_t depth;             // >= 1
    int mode;                   // kLfModeAll / Same / Different
    uint64_t ignore;            // the label of an unlabelled node
    int b;                      // bits per node id: a key is source << b | node
    uint32_t* queue;            // per wave qstride words: its node list past the LDS part
    uint32_t qstride;
    uint32_t* bits;             // per wave bstride words: a bitmap over the nodes, zero between sources
    uint32_t bstride;
    uint64_t* keys;             // out
    unsigned long long cap;     // keys at positions >= cap are counted, not written
    unsigned long long* count;  // the append counter
    unsigned long long* visits; // the adjacency entries looked at, summed over the waves
};
__global__ void k_lf_degrees(const uint64_t*, uint32_t, uint64_t, uint32_t*, unsigned long long*);
__global__ void k_lf_fill(const uint64_t*, uint32_t, const uint32_t*, uint32_t*, uint32_t*);
__global__ void k_lf_sources(const uint64_t*, uint32_t, uint64_t, uint32_t*, unsigned long long*);
__global__ void k_lf_bfs(LfArgs);
__global__ void k_lf_unpack(const uint64_t*, int64_t, int, uint64_t*);
// k_graphpost.hip (ConnectedComponentsWorkflow, SizeFilterAndGraphWatershedWorkflow: graph components
// and the seeded graph watershed over an edge table)
constexpr int kGpMaxIters = 34;  // rounds of a watershed, and pointer-jumping passes of a round: then an error
// the words of the edge checks' counter block
constexpr int kGpBadId = 0, kGpBadNan = 1;
__global__ void k_gp_init(uint32_t*, uint32_t*, uint64_t);
__global__ void k_gp_union(const uint64_t*, uint64_t, uint64_t, const uint64_t*, uint32_t*, unsigned long long*);
__global__ void k_gp_compress(uint32_t*, uint64_t);
__global__ void k_gp_cc_flag(const uint32_t*, const uint64_t*, uint64_t, uint32_t*);
__global__ void k_gp_cc_write(const uint32_t*, const uint64_t*, const uint32_t*, uint64_t, uint64_t*);
__global__ void k_gp_keys(const uint64_t*, const double*, uint64_t, uint64_t, uint64_t*, uint32_t*, unsigned long long*);
__global__ void k_gp_sorted_ends(const uint64_t*, const uint32_t*, uint64_t, uint32_t*, uint32_t*);
__global__ void k_gp_offer(uint32_t*, const uint32_t*, uint64_t, const uint32_t*, const uint64_t*, uint32_t*);
__global__ void k_gp_hook(const uint32_t*, const uint32_t*, const uint32_t*, const uint64_t*, const uint32_t*, uint32_t*,
                          uint64_t, unsigned long long*);
__global__ void k_gp_jump(uint32_t*, uint32_t*, uint64_t, unsigned long long*);
__global__ void k_gp_ws_write(const uint32_t*, const uint64_t*, uint64_t, uint64_t*);
__global__ void k_gp_rl_keys(const uint64_t*, uint64_t, uint64_t*, uint32_t*, uint32_t*);
__global__ void k_gp_rl_heads(const uint64_t*, const uint32_t*, uint64_t, uint32_t*);
__global__ void k_gp_rl_write(const uint64_t*, const uint32_t*, const uint32_t*, uint64_t, uint64_t*);

// k_prims.hip (the device-wide primitives of the feature calls; tmp == nullptr: only size bytes)
hipError_t sort_keys_u64(void* tmp, size_t& bytes, const uint64_t* keys_in, uint64_t* keys_out, int64_t n,
                         int end_bit, hipStream_t stream);
hipError_t sort_pairs_u64(void* tmp, size_t& bytes, const uint64_t* keys_in, uint64_t* keys_out,
                          const uint64_t* vals_in, uint64_t* vals_out, int64_t n, int end_bit, hipStream_t stream);
hipError_t sort_pairs_u64_u32(void* tmp, size_t& bytes, const uint64_t* keys_in, uint64_t* keys_out,
                              const uint32_t* vals_in, uint32_t* vals_out, int64_t n, hipStream_t stream);
hipError_t exclusive_sum_u32(void* tmp, size_t& bytes, const uint32_t* in, uint32_t* out, int64_t n,
                             hipStream_t stream);
hipError_t runs_u64(void* tmp, size_t& bytes, const uint64_t* sorted, uint64_t* uniq, uint64_t* counts,
                    uint64_t* n_runs, int64_t n, hipStream_t stream);
hipError_t reduce_by_key_sum_u64(void* tmp, size_t& bytes, const uint64_t* keys, uint64_t* uniq,
                                 const uint64_t* vals, uint64_t* sums, uint64_t* n_runs, int64_t n, hipStream_t stream);

// k_threshcc.hip (ThresholdedComponents: BlockComponents)
struct TcParams {
    int nz, ny, nx;
    int mode;       // 0 greater, 1 less, 2 equal
    int normalize;  // 1: vu.normalize before the threshold (min / max from k_tc_minmax)
    float thr;      // the threshold as float32
};
__global__ void k_tc_minmax(const float*, int64_t, uint32_t*);
__global__ void k_tc_tile(const float*, const uint8_t*, TcParams, const uint32_t*, uint32_t*, uint32_t*);
__global__ void k_tc_merge(TcParams, uint32_t*);
__global__ void k_tc_roots(const uint32_t*, int64_t, uint64_t*);
__global__ void k_tc_wordoff(const uint64_t*, int64_t, const uint64_t*, uint32_t*);
__global__ void k_tc_label(const uint32_t*, int64_t, const uint64_t*, const uint32_t*, uint64_t*);
template <class T>
__global__ void k_tc_to_f32(const T*, int64_t, float*);
template <class T>
__global__ void k_tc_raw_members(const T*, int64_t, int, double, float*);
__global__ void k_tc_normalize(float*, int64_t, const uint32_t*);
__global__ void k_tc_gauss(const float*, float*, int, int, int, int, const double*, int);

// k_imgfilter.hip (ImageFilter: Gaussian smoothing, gradient magnitude, Laplacian of Gaussian)
constexpr int kIfMaxR = 48;    // largest tap radius: 2 inputs x (kIfColTL + 2 kIfMaxR) x kIfColW floats = 64 KiB of LDS
constexpr int kIfColTL = 32;   // column pass: outputs along the axis per tile
constexpr int kIfColW = 64;    // column pass: x positions per tile (a wave's lanes)
constexpr int kIfRowW = 256;   // row pass: outputs per row segment (4 per lane)
constexpr int kIfSmooth = 0, kIfGradMag = 1, kIfLaplace = 2;
struct IfArgs {
    const void* in[3];    // column pass: NIN arrays of the kernel's type T; row pass: NIN float arrays
    float* out[3];        // column pass: NOUT arrays; row pass: out[0]
    int tap[3], rad[3];   // first tap (offset -rad) in taps and radius, per output (column) or per input (row)
    const double* taps;
    const uint32_t* mm;   // normalize: ordered-float bits of the block's min and max (k_if_minmax)
    int normalize;        // 1: the pass reads (float(x) - min) / fl(max - min), vu.normalize on the fly
    int nz, ny, nx;       // nz * ny * nx < 2^31
    int axis;             // column pass: 0 (z) or 1 (y)
    int rmax;             // max over rad: the tile's halo (every line holds at least rmax + 1 voxels)
    int combine;          // row pass: kIfSmooth the one result, kIfGradMag sqrt of the squares' sum, kIfLaplace the sum
};
template <class T>
__global__ void k_if_minmax(const T*, int64_t, uint32_t*);
// outputs of a column pass: NIN = 1: all of input 0; NIN = 2: output 0 of input 0, outputs 1, 2 of input 1
template <class T, int NIN, int NOUT>
__global__ void k_if_col(IfArgs);
template <int NIN>
__global__ void k_if_row(IfArgs);

}  // namespace ctws
