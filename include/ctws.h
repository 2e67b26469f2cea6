/*
 * ctws.h — C-ABI of libctws.so, the MI355X (gfx950) blockwise DT-watershed.
 *
 * This is the drop-in boundary for the hot path of cluster_tools' watershed task.
 * Every entry point is plain C: pointers, sizes, POD structs.  No torch / HIP types.
 *
 * Reference interfaces each entry point replaces (paths relative to the reference repo):
 *
 *   ctws_ws_blocks / ctws_ws_blocks_device
 *       the per-job block loop `for block_id in block_list: _ws_block(...)`
 *       cluster_tools/watershed/watershed.py:380-381, i.e. `_ws_block` (:285-341) with
 *       `_read_data` (:267-282), `_apply_dt` (:139-160), `_make_seeds` (:179-207),
 *       `_make_hmap` (:163-169), `_apply_watershed` (:211-249) and the halo crop /
 *       labelVolumeWithBackground / id offset (:326-341);
 *       and, with cfg.pass_id == 1, `_ws_pass2`
 *       cluster_tools/watershed/two_pass_watershed.py:210-255 (+ :122-207).
 *       The caller does the dataset I/O (ds_in[input_bb], ds_out[output_bb] = ...) and the
 *       "processed block" log lines, exactly as the reference job entry does.
 *
 *   ctws_ws_from_seeds / ctws_ws_from_seeds_device
 *       the WatershedFromSeeds job loop (watershed/watershed_from_seeds.py:236-249 over
 *       `_ws_block` / `_ws_block_masked`, :143-199).
 *
 *   ctws_eval_begin / ctws_eval_add / ctws_eval_end
 *       EvaluationWorkflow's overlaps + Measures (evaluation/evaluation_workflow.py:53-77,
 *       evaluation/measures.py:80-164, utils/validation_utils.py:60-76, 178-198).
 *
 *   ctws_threshold_components / ctws_ufd_find
 *       ThresholdedComponentsWorkflow: BlockComponents' per-block `_cc_block[_with_mask]`
 *       (thresholded_components/block_components.py:143-230: normalize, threshold,
 *       skimage.morphology.label) and MergeAssignments' nifty boost_ufd merge + find
 *       (thresholded_components/merge_assignments.py:125-130).
 *
 *   ctws_open / ctws_close / ctws_last_error
 *       process-level setup; the reference has none (vigra is stateless).  One handle per
 *       (process, GPU), as LocalTask runs one process per job (cluster_tasks.py:507-529).
 *
 *   (multi-GPU) the library holds no communicator: the per-block label counts it returns
 *       (ctws_block.n_ids) are all-gathered and exclusively scanned by the host over
 *       torch.distributed (RCCL, cluster_tools_amd/watershed/sharded.py), replacing the
 *       FindUniques -> FindLabeling file exchange (relabel/find_labeling.py:104-116,
 *       thresholded_components/merge_offsets.py:111-119).
 *
 * Conventions
 *   - all arrays are C-contiguous numpy-order arrays (axis 0 = z slowest, axis 2 = x fastest)
 *   - the caller owns every buffer it passes; no pointer is retained after return
 *   - return value 0 = ok, negative = error; the message is in ctws_last_error(h)
 *   - calls on one handle are serialized (not re-entrant); use one handle per thread
 */
#ifndef CTWS_H
#define CTWS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTWS_ABI_VERSION 2

/* error codes */
#define CTWS_OK            0
#define CTWS_EINVAL       -1  /* bad argument                                    */
#define CTWS_EHIP         -2  /* HIP runtime error                               */
#define CTWS_ENOMEM       -3  /* device allocation failed                        */
#define CTWS_ECOMM        -4  /* RCCL error                                      */
#define CTWS_EUNSUPPORTED -5  /* configuration the kernels do not implement      */

/* input dtypes (ds_in dtype; the reference casts to float32 in normalize) */
#define CTWS_U8  1
#define CTWS_U16 2
#define CTWS_F32 3
#define CTWS_F64 4
/* further dtypes of ctws_threshold_components_ex (BlockComponents thresholds the raw dataset) */
#define CTWS_I8  5
#define CTWS_I16 6
#define CTWS_I32 7
#define CTWS_U32 8
#define CTWS_I64 9
#define CTWS_U64 10

/* agglomerate_channels */
#define CTWS_AGG_MEAN 0
#define CTWS_AGG_MAX  1
#define CTWS_AGG_MIN  2

/* per-block status written by ctws_ws_blocks */
#define CTWS_BLOCK_WRITTEN      0  /* output holds the block's uint64 labels           */
#define CTWS_BLOCK_SKIPPED_MASK 1  /* inner mask empty: nothing written (:295-297)     */
#define CTWS_BLOCK_EMPTY        2  /* nothing above threshold: constant offset written */
#define CTWS_BLOCK_EMPTY_PASS2  3  /* pass 2, nothing above threshold: nothing written */
#define CTWS_BLOCK_FAILED       4  /* the block cannot be finished: nothing written;    */
                                   /* the reason is in ctws_last_error (the reference   */
                                   /* job would raise at this block)                    */
/* further statuses of ctws_size_filter_blocks */
#define CTWS_BLOCK_ZERO         5  /* every label is 0: nothing written                 */
#define CTWS_BLOCK_COPIED       6  /* no voxel carries a discard id: output = labels    */

/*
 * Task configuration.  Mirrors the watershed task config keys
 * (watershed.py:50-60, two_pass_watershed.py:39-49) with the inline defaults the job
 * code applies (config.get(k, default)).
 */
typedef struct ctws_cfg {
    double  threshold;               /* 'threshold' (compared in float32)                  */
    double  alpha;                   /* 'alpha'                                            */
    double  sigma_seeds[3];          /* 'sigma_seeds': scalar in [0] or per-axis list      */
    int32_t sigma_seeds_is_list;     /*   1 if the config held a list/tuple                */
    double  sigma_weights[3];        /* 'sigma_weights'                                    */
    int32_t sigma_weights_is_list;
    int32_t size_filter;             /* 'size_filter'                                      */
    int32_t apply_dt_2d;             /* 'apply_dt_2d'                                      */
    int32_t apply_ws_2d;             /* 'apply_ws_2d'                                      */
    int32_t has_pixel_pitch;         /* 'pixel_pitch' is not None                          */
    double  pixel_pitch[3];
    int32_t invert_inputs;           /* 'invert_inputs'                                    */
    int32_t channel_begin;           /* 'channel_begin'                                    */
    int32_t channel_end;             /* 'channel_end', < 0 means None (every channel): NOT */
                                     /* python's negative index.  A config's negative end  */
                                     /* (slice(b, -1) drops the last channel) has to be    */
                                     /* resolved by the caller; _abi.make_cfg refuses it   */
    int32_t agglomerate_channels;    /* CTWS_AGG_*                                         */
    int32_t non_maximum_suppression; /* must be 0: nifty NMS is not available (:20-23)     */
    int32_t pass_id;                 /* 0 = _ws_block, 1 = _ws_pass2                       */
    int64_t block_shape[3];          /* global block shape: offset = id * prod(shape)      */
} ctws_cfg;

/*
 * One block.  `input` holds the OUTER block (block + halo, clipped to the volume) as
 * ds_in[input_bb] would return it; `output` receives ws[inner_bb] as uint64.
 */
typedef struct ctws_block {
    const void*     input;           /* [C][Z][Y][X] (n_channels > 0) or [Z][Y][X]         */
    int32_t         input_dtype;     /* CTWS_U8 / U16 / F32 / F64                          */
    int32_t         n_channels;      /* 0 for a 3-D dataset                                */
    int64_t         outer_shape[3];  /* Z, Y, X of the outer block                         */
    const uint8_t*  mask;            /* outer-shaped, nonzero = in mask; NULL = no mask    */
    int64_t         inner_begin[3];  /* inner block, local to the outer block              */
    int64_t         inner_shape[3];
    int32_t         crop_relabel;    /* 1 iff output_bb != input_bb (:327)                 */
    int32_t         _pad0;
    int64_t         block_id;        /* id offset = block_id * prod(cfg.block_shape)       */
    const uint64_t* initial_seeds;   /* pass 2: ds_out[input_bb], outer-shaped; else NULL  */
    uint64_t*       output;          /* inner-shaped uint64                                */
    uint64_t        max_label;       /* out: largest local label before the id offset      */
    int32_t         status;          /* out: CTWS_BLOCK_*                                  */
    int32_t         n_ids;           /* out: distinct nonzero output ids of the block (pass */
                                     /* 0; -1 in pass 2): the per-block count of the       */
                                     /* compact-id exclusive scan (find_labeling.py:104)   */
} ctws_block;

typedef struct ctws_handle ctws_handle;

/* version of this header the library was built against */
int ctws_abi_version(void);

/* open the library on HIP device `device` (index within HIP_VISIBLE_DEVICES) */
int ctws_open(int device, ctws_handle** out);
void ctws_close(ctws_handle* h);
const char* ctws_last_error(const ctws_handle* h);

/*
 * Run the watershed of `n_blocks` blocks.  input/mask/initial_seeds/output are HOST
 * pointers.  The blocks run in device-memory-sized batches; each batch's inputs are packed
 * (multi-threaded memcpy) into one of two pinned host buffers and uploaded on a copy stream
 * while the previous batch computes, and its outputs are downloaded on a second copy stream
 * and unpacked while the next batch computes.  The pinned and device staging buffers are kept
 * by the handle (grow-only) for later calls.
 */
int ctws_ws_blocks(ctws_handle* h, const ctws_cfg* cfg, ctws_block* blocks, int n_blocks);

/*
 * Same, but input/mask/initial_seeds/output are DEVICE pointers on the handle's GPU
 * (e.g. torch tensors' data_ptr()).  Work is enqueued on the handle's stream and the
 * call returns after the stream has drained.
 */
int ctws_ws_blocks_device(ctws_handle* h, const ctws_cfg* cfg, ctws_block* blocks, int n_blocks);

/*
 * WatershedFromSeeds (watershed/watershed_from_seeds.py:143-199, `_ws_block` and
 * `_ws_block_masked`): per block, input = normalize(ds_in[bb]) (4-D: channel range +
 * agglomeration; no invert), masked voxels -> 1, seeds = `initial_seeds` (= ds_seeds[bb],
 * uint64, the block's shape), ws = watershedsNew(input, seeds) (3-D, direct nbhd) + the
 * size filter (cfg.size_filter), ws[~mask] = 0 -> `output` (uint64).  Blocks have no halo:
 * inner_begin = 0, inner_shape = outer_shape.  Only threshold-independent keys of `cfg` are
 * read (size_filter, channel_begin/end, agglomerate_channels).  A block whose seeds hold an
 * id >= 2^32 - 1 gets CTWS_BLOCK_FAILED (the reference's "Overflow detected" assert); a block
 * with an empty mask CTWS_BLOCK_SKIPPED_MASK (nothing written).  max_label = largest output id.
 */
int ctws_ws_from_seeds(ctws_handle* h, const ctws_cfg* cfg, ctws_block* blocks, int n_blocks);
int ctws_ws_from_seeds_device(ctws_handle* h, const ctws_cfg* cfg, ctws_block* blocks, int n_blocks);

/*
 * SizeFilterWorkflow (postprocess/postprocess_workflow.py:24-112): the block loops of
 * BackgroundSizeFilter (background_size_filter.py:110-130) and FillingSizeFilter
 * (filling_size_filter.py:112-136, `apply_block`).
 *
 * ctws_set_discard_u64: upload the discard ids (host, strictly ascending; discard_ids.npy of
 *   SizeFilterBlocks) and keep them resident on the handle; n = 0 clears the set.  The set is a
 *   sorted table, and a bitmap over [ids[0], ids[n - 1]] too when that range is below 2^28.
 * ctws_size_filter_blocks / _device: per block, `initial_seeds` = the block's uint64 labels
 *   (ds_in[bb]; no halo: inner_begin = 0, inner_shape = outer_shape), `output` = the uint64
 *   result (may be the labels' own buffer), and with fill = 1 `input` = the RAW height map of
 *   the block (CTWS_U8 / U16 / F32, n_channels 0; a float64 or multi-channel map gives
 *   CTWS_BLOCK_FAILED with the reason).  Host pointers, or device pointers for _device.
 *     every label 0              -> CTWS_BLOCK_ZERO, nothing written
 *     no voxel in the discard set -> CTWS_BLOCK_COPIED, output = labels
 *     else                        -> CTWS_BLOCK_WRITTEN: labels with the discarded ids set to 0
 *       (fill = 0), or watershedsNew(float32(input), seeds = those labels) (fill = 1; 3-D direct
 *       nbhd; the height map is NOT normalized and the ids keep their full 64 bits, flooded as
 *       order-preserving compact labels; a block without any label left is seeded by vigra
 *       from the strict minima of the height map and gets ids 1..n, as in the reference).
 *   max_label = the largest output id.  The only reserved id is 2^64 - 1 (fill = 1:
 *   CTWS_BLOCK_FAILED).  mask, block_id (messages only) and cfg-like fields are not read.
 */
int ctws_set_discard_u64(ctws_handle* h, const uint64_t* ids, int64_t n);
int ctws_size_filter_blocks(ctws_handle* h, ctws_block* blocks, int n_blocks, int fill);
int ctws_size_filter_blocks_device(ctws_handle* h, ctws_block* blocks, int n_blocks, int fill);

/*
 * Evaluation (evaluation/measures.py:80-164 with utils/validation_utils.py:60-76, 178-198):
 * the seg x gt contingency table built in HBM (hash tables of gt ids, seg ids and id pairs
 * with voxel counts), accumulated over any number of ctws_eval_add calls (blockwise), then
 * reduced.  cap_labels / cap_pairs bound the distinct ids per side / distinct pairs; a full
 * table makes ctws_eval_end return CTWS_EUNSUPPORTED (retry with larger capacities).
 * ignore_gt_zero drops voxels whose gt label is 0 (EvaluationWorkflow(ignore_label=True),
 * evaluation_workflow.py:53,60).  scores = {vi_split, vi_merge, adapted_rand_error,
 * rand_index} (log2), exactly the keys measures() writes.
 */
int ctws_eval_begin(ctws_handle* h, int64_t cap_labels, int64_t cap_pairs);
int ctws_eval_add(ctws_handle* h, const uint64_t* seg, const uint64_t* gt, int64_t n, int on_device,
                  int ignore_gt_zero);
int ctws_eval_end(ctws_handle* h, double* scores /* [4] */, int64_t* n_points);

/*
 * Stage timings of the last ctws_ws_blocks* call, measured with HIP events on the
 * handle's stream (milliseconds).  names[i] is a static string.  Returns the count.
 * Some entries are counters, not times, summed over the call's batches (flood_rounds,
 * flood_packed, sf_sparse_blocks, sf_redo_blocks, hist_fused, seed_dense, host_batches, ...).  One names a kernel and is
 * that of the call's last batch: prep_kernel, the normalize + EDT x pass --
 *     0            the generic LDS row kernel k_prep_edt_x (4-D input, rows > 1024 voxels,
 *                  blocks of different dtypes in one batch) with the generic k_input_minmax
 *     4, 8, 16     k_prep_edt_x_co<KMAX, T, false>
 *     104, 108, 116  k_prep_edt_x_co<KMAX, T, true> (foreground bits for the y pass)
 *     204, 208, 216  k_prep_edt_x_reg<KMAX> (float32 rows of exactly 256 / 512 / 1024 voxels)
 *     -1           the filling size filter (no prep pass: the height map as stored)
 * The typed k_input_minmax_t<T> ran exactly when the value is positive.
 */
int ctws_last_timings(const ctws_handle* h, const char** names, float* ms, int max_entries);

/*
 * RelabelWorkflow (relabel/find_uniques.py:93-159, find_labeling.py:84-126,
 * write/write.py:153-226) on the GPU.  on_device = 1: labels/out/keys/values are device
 * pointers on the handle's GPU; 0: host pointers (staged through HBM).
 *
 * ctws_unique_u64: the sorted unique values of labels[0..n) (np.unique) into out[0..cap);
 *   *n_unique = their number (also when cap is too small: then CTWS_EINVAL, retry with a
 *   larger buffer).  Any value range: a bitmap over the range when it is dense enough
 *   (watershed ids), else a radix sort.  Fewer than 2^31 labels per call.
 * ctws_unique_counts_u64: np.unique(labels, return_counts=True) (find_uniques.py:104-106):
 *   sorted uniques into out, their voxel counts into counts (both cap entries).
 * ctws_set_table_u64: upload an assignment table (host keys ascending, values) and keep it
 *   resident on the handle (one upload per Write job instead of one per block).
 * ctws_lookup_u64: labels[i] <- values[j] where keys[j] == labels[i] (keys ascending;
 *   nifty.tools.takeDict); labels absent from the table are left unchanged and counted in
 *   *n_missing (takeDict would raise: the caller raises).  keys == values == NULL: use the
 *   resident table; host keys/values (on_device = 0) become the resident table.
 */
int ctws_set_table_u64(ctws_handle* h, const uint64_t* keys, const uint64_t* values, int64_t n_table);
int ctws_unique_u64(ctws_handle* h, const uint64_t* labels, int64_t n, int on_device, uint64_t* out, int64_t cap,
                    int64_t* n_unique);
int ctws_unique_counts_u64(ctws_handle* h, const uint64_t* labels, int64_t n, int on_device, uint64_t* out,
                           uint64_t* counts, int64_t cap, int64_t* n_unique);
int ctws_lookup_u64(ctws_handle* h, uint64_t* labels, int64_t n, int on_device, const uint64_t* keys,
                    const uint64_t* values, int64_t n_table, int64_t* n_missing);

/*
 * GraphWorkflow (graph/graph_workflow.py:9-72): the region adjacency graph of the fragments.
 *
 * ctws_rag_block / _device: the graph of one block of uint64 labels, shape (nz, ny, nx), C order
 *   -- the extended box [block.begin, min(block.end + 1, shape)) of InitialSubGraphs
 *   (initial_sub_graphs.py:106-120, `ndist.computeMergeableRegionGraph(..., increaseRoi=True)`).
 *     nodes   the sorted unique labels (np.unique), without 0 when ignore_label is set
 *     edges   the sorted set of (min(u, v), max(u, v)) over all face-adjacent voxel pairs of the
 *             block with u != v -- and u != 0, v != 0 when ignore_label is set -- as m x 2
 *             (`nrag.gridRag(seg).uvIds()`, test/graph/test_graph.py:63-126)
 *     counts  per edge the number of such voxel pairs; may be NULL
 *   *n_nodes and *n_edges are always set; CTWS_EINVAL when cap_nodes or cap_edges is too small
 *   (nothing written: retry with those sizes).  Every uint64 value is a legal id.  Fewer than
 *   2^31 voxels per block.  Host pointers are staged through HBM; _device takes device pointers
 *   on the handle's GPU for labels, nodes, edges and counts.
 * ctws_unique_pairs_u64: the lexicographically sorted unique rows of pairs (n x 2) into out
 *   (cap x 2) with the sum of their weights (weights == NULL: 1 each) into counts (cap entries, or
 *   NULL) -- the edge part of `ndist.mergeSubgraphs` (merge_sub_graphs.py:133-158) on the
 *   concatenated edge tables of the children.  *n_unique is always set; CTWS_EINVAL when cap is
 *   too small.  on_device as for ctws_unique_u64.  Fewer than 2^30 pairs and 2^32 distinct
 *   values per call (CTWS_EUNSUPPORTED otherwise).
 */
int ctws_unique_pairs_u64(ctws_handle* h, const uint64_t* pairs, const uint64_t* weights, int64_t n, int on_device,
                          uint64_t* out, uint64_t* counts, int64_t cap, int64_t* n_unique);
int ctws_rag_block(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx, int ignore_label,
                   uint64_t* nodes, int64_t cap_nodes, int64_t* n_nodes, uint64_t* edges, uint64_t* counts,
                   int64_t cap_edges, int64_t* n_edges);
int ctws_rag_block_device(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx,
                          int ignore_label, uint64_t* nodes, int64_t cap_nodes, int64_t* n_nodes, uint64_t* edges,
                          uint64_t* counts, int64_t cap_edges, int64_t* n_edges);

/*
 * NodeLabelWorkflow (node_labels/node_label_workflow.py), BlockNodeLabels: the overlaps of the
 * fragments with a second label volume (block_node_labels.py:130-170,
 * `ndist.computeAndSerializeLabelOverlaps`, restated: DESIGN.md section 3.6).
 *
 * ctws_label_overlaps / _device: nodes_vol and labels_vol are two uint64 arrays of n voxels each;
 *   only the voxel correspondence matters, so there is no shape.
 *     rows    m x 3 uint64, C order: (node, label, count) for every pair that occurs at a counted
 *             voxel, sorted lexicographically by (node, label); count = the voxels with that pair
 *     with_ignore != 0: voxels whose LABEL equals ignore_label are not counted (`withIgnoreLabel`
 *             / `ignoreLabel`, block_node_labels.py:153-156).  Voxels of node 0 are counted like
 *             any other.
 *   *n_rows is always set; CTWS_EINVAL when cap (in rows) is too small (nothing written: retry
 *   with that size).  Every uint64 value is a legal id on both sides, 2^64 - 1 included.  The rows
 *   depend on the inputs alone (repeated calls agree byte for byte).  Fewer than 2^31 voxels, 2^30
 *   runs of equal pairs in scan order and 2^32 distinct values (node and label ids together) per
 *   call: the limits of the path behind ctws_unique_pairs_u64, which sorts and sums the runs
 *   (CTWS_EUNSUPPORTED otherwise).  Host pointers are staged through HBM; _device takes device
 *   pointers on the handle's GPU for nodes_vol, labels_vol and rows.
 */
int ctws_label_overlaps(ctws_handle* h, const uint64_t* nodes_vol, const uint64_t* labels_vol, int64_t n,
                        int with_ignore, uint64_t ignore_label, uint64_t* rows, int64_t cap, int64_t* n_rows);
int ctws_label_overlaps_device(ctws_handle* h, const uint64_t* nodes_vol, const uint64_t* labels_vol, int64_t n,
                               int with_ignore, uint64_t ignore_label, uint64_t* rows, int64_t cap, int64_t* n_rows);

/*
 * MorphologyWorkflow (morphology/morphology_workflow.py:11-56), BlockMorphology: size, centre of
 * mass and bounding box of every id of a block (block_morphology.py:111-136,
 * `ndist.computeAndSerializeMorphology`, restated: DESIGN.md section 3.7).
 *
 * ctws_block_morphology / _device: labels is one block of uint64 ids, shape (nz, ny, nx), C order;
 *   begin (three values, always a host pointer) is the block's offset in the volume.
 *     rows    m x 11 float64, C order, a row per id that occurs in the block -- 0 included, there is
 *             no ignore label -- sorted by id:
 *             [id, n, com_z, com_y, com_x, min_z, min_y, min_x, max_z, max_y, max_x] over the id's
 *             voxels at the global coordinates g = begin + local: n = their number, com_a =
 *             float64(sum of g_a) / float64(n) with the sum taken in integers (one IEEE division),
 *             min_a and max_a both inclusive.  A block of zeros gives the one row of id 0 (the rule
 *             that skips such a block is the task's).
 *   *n_rows is always set; CTWS_EINVAL when cap (in rows) is too small (nothing written: retry
 *   with that size) or a begin is negative.  Ids below 2^53 (the id column is exact), every extent
 *   below 2^19, fewer than 2^31 voxels and begin + extent <= 2^21 per axis (every coordinate sum
 *   stays below 2^52 and converts exactly): CTWS_EUNSUPPORTED otherwise, never a wrong row.  The
 *   accumulation is integer throughout, so the rows depend on the inputs alone (repeated calls
 *   agree byte for byte).  Host pointers are staged through HBM; _device takes device pointers on
 *   the handle's GPU for labels and rows.
 */
int ctws_block_morphology(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx,
                          const int64_t begin[3], double* rows, int64_t cap, int64_t* n_rows);
int ctws_block_morphology_device(ctws_handle* h, const uint64_t* labels, int64_t nz, int64_t ny, int64_t nx,
                                 const int64_t begin[3], double* rows, int64_t cap, int64_t* n_rows);

/*
 * RegionFeaturesWorkflow (features/features_workflow.py:71-112), RegionFeatures: the number of
 * voxels and the mean input value of every id of a block (region_features.py:122-167,
 * `vigra.analysis.extractRegionFeatures(..., ['mean', 'count'], ignoreLabel=...)` on
 * `vu.normalize(input)`, restated: DESIGN.md section 3.8).
 *
 * ctws_region_features_block / _device: labels (uint64) and data (data_dtype CTWS_U8 / U16 / F32 /
 *   F64) are one block, shape (nz, ny, nx), C order.  The value of a voxel is float32: uint8 gives
 *   float32(v) / 255.0f, uint16 and float32 give float32(v) (uint16 is not scaled), float64 is
 *   rounded to nearest.  NaN values are not supported (an id that holds one gets a NaN mean).
 *     rows    m x 3 float64, C order, a row per id that occurs in the block, sorted by id:
 *             [id, n, mean], n = the id's number of voxels, mean = float64(sum) / float64(n) with
 *             one IEEE division, sum = the float64 sum of the id's float32 values.  With
 *             with_ignore != 0 the row of ignore_label, if that id occurs, is [ignore_label, 0, 0];
 *             a block that holds nothing else gives that single row (the rule that skips such a
 *             block is the task's).
 *   *n_rows is always set; CTWS_EINVAL when cap (in rows) is too small (nothing written: retry
 *   with that size) or data_dtype is none of the four.  Ids below 2^53 (the id column is exact)
 *   and fewer than 2^31 voxels in fewer than 2^31 - 1 rows (nz * ny): CTWS_EUNSUPPORTED
 *   otherwise, never a wrong row.  The sum of an id is taken in an order that follows from the labels alone -- no floating-point atomic, no
 *   dependence on the order in which waves run -- so the rows depend on the inputs alone: repeated
 *   calls, and the host- and device-pointer forms, agree byte for byte.  Its error against the
 *   exact sum is that of a float64 sum of n terms in some order, at most (n - 1) 2^-53 sum|x|.
 *   Host pointers are staged through HBM; _device takes device pointers on the handle's GPU for
 *   labels, data and rows.
 */
int ctws_region_features_block(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype, int64_t nz,
                               int64_t ny, int64_t nx, int with_ignore, uint64_t ignore_label, double* rows,
                               int64_t cap, int64_t* n_rows);
int ctws_region_features_block_device(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype,
                                      int64_t nz, int64_t ny, int64_t nx, int with_ignore, uint64_t ignore_label,
                                      double* rows, int64_t cap, int64_t* n_rows);

/*
 * DownscalingWorkflow (downscaling/downscaling_workflow.py:218-347), Downscaling with
 * `library: 'skimage'`: one block of one level of a scale pyramid (downscaling.py:222-229 `_ds_vol`
 * over :309-310 `block_reduce`, restated: DESIGN.md section 3.9).
 *
 * ctws_downscale_block / _device: input = one block (nz, ny, nx), C order, of dtype CTWS_U8,
 *   CTWS_U16, CTWS_F32 or CTWS_F64; factors = (fz, fy, fx), each 1..8; func 0 mean, 1 max, 2 min.
 *   out (oz, oy, ox) = (ceil(nz / fz), ceil(ny / fy), ceil(nx / fx)), C order, in the input's
 *   dtype; the caller passes the extents, any other is CTWS_EINVAL.
 *     cell    out[z, y, x] reduces input[z fz .. (z + 1) fz, y fy .., x fx ..]; the input is
 *             zero-padded at the end of every axis to a multiple of its factor, and the zeros take
 *             part: the mean divides by n = fz fy fx, a padded cell's min is <= 0, its max >= 0.
 *     value   float64 is rounded to float32 (to nearest) first; every dtype is reduced as float32
 *     mean    float32(S) / float32(n), one IEEE float32 division.  Integers: S is the cell's exact
 *             integer sum; then clip to the dtype's range, round half to even, cast.  A uint16 mean
 *             with n > 256 (n 65535 >= 2^24: float32 no longer holds S, the reference's float32
 *             summation order would decide) is CTWS_EUNSUPPORTED.  Floats: S is the float64 sum in
 *             the order z, then y, then x ascending, rounded once to float32; float64 output is the
 *             float32 result widened.
 *     max/min exact.
 *   *any_nonzero = 0 when every input voxel is zero (-0.0 is zero), else 1: the reference's
 *   `np.sum(x != 0) == 0` skip test, taken in the same pass.  out is written either way.
 *   NaN inputs are not supported.  No floating-point atomics: the output depends on the input
 *   alone, so repeated calls, and the host- and device-pointer forms, agree byte for byte.
 *   Fewer than 2^31 voxels per block: more is CTWS_EUNSUPPORTED before any memory is touched.
 *   Host pointers are staged through HBM; _device takes device pointers on the handle's GPU for
 *   input and out (any_nonzero stays a host pointer).  A 4-D volume is one call per channel.
 */
int ctws_downscale_block(ctws_handle* h, const void* input, int dtype, int64_t nz, int64_t ny, int64_t nx,
                         const int64_t factors[3], int func, void* out, int64_t oz, int64_t oy, int64_t ox,
                         int* any_nonzero);
int ctws_downscale_block_device(ctws_handle* h, const void* input, int dtype, int64_t nz, int64_t ny, int64_t nx,
                                const int64_t factors[3], int func, void* out, int64_t oz, int64_t oy, int64_t ox,
                                int* any_nonzero);

/*
 * RegionCentersWorkflow (morphology/morphology_workflow.py:59-112), RegionCenters: per object the
 * voxel of its box that is farthest from the box's background (region_centers.py:106-133,
 * `np.argmax(distance_transform_edt(labels[box] == id, sampling=resolution))`, restated: DESIGN.md
 * section 3.10).
 *
 * ctws_region_centers / _device: labels is one buffer of n_labels uint64 ids that holds the boxes
 *   of k objects.  Object i is ids[i], offsets[i] (of the box's first voxel, in elements),
 *   shapes[3 i ..] = (nz, ny, nx) and pitches[2 i ..] = (z pitch, y pitch) in elements, x
 *   contiguous: packed crops one after another (pitches (ny nx, nx)) and boxes inside one resident
 *   volume (the volume's pitches) are the same call.  ids, offsets, shapes, pitches and resolution
 *   are always host pointers.
 *     d2      of a voxel p with label == ids[i] (all 64 bits compare): the minimum over the box's
 *             voxels b with another label of sum_a (resolution[a] (p_a - b_a))^2, an exact integer;
 *             0 for the other voxels.  Only voxels inside the box count as background.
 *     centers k x 3 int64, C order: the local (z, y, x) of the first voxel in C order of the box with
 *             the largest d2.  A box without background gives its last voxel, shape - 1 (scipy
 *             1.15 treats such a box as if one background voxel sat at local (-1, 0, 0)).
 *     found   k x uint8: 0 when the box is empty (an extent of 0) or holds no voxel of the id; the
 *             centre is then (0, 0, 0).
 *   Limits, CTWS_EUNSUPPORTED otherwise and never a wrong centre: every resolution an integer in
 *   1 .. 2^10 (given as double; with a non-integer value the reference's float64 roundings decide
 *   ties, which is not restated; the centre does not change when all three values are scaled by a
 *   common factor); sum_a (resolution[a] shape[a])^2 < 2^31 per box (d2 is 32-bit); fewer than 2^31
 *   voxels per box; fewer than 2^31 objects.  CTWS_EINVAL for a box that does not lie inside the
 *   buffer, rows that overlap (y pitch < nx, z pitch < (ny - 1) y pitch + nx) or a negative value;
 *   nothing is launched then.
 *   Boxes of at most 10000 voxels run one workgroup each, all in one launch, with the transform in
 *   LDS; larger boxes run separable passes through scratch memory of the handle (8 bytes per box
 *   voxel, in groups of at most 2^28 voxels).  ctws_last_timings reports rc_small_objects and
 *   rc_large_objects.  The maximum is taken over integer keys (d2, first index): the result
 *   depends on the inputs alone, repeated calls agree byte for byte.  Host pointers are staged
 *   through HBM; _device takes device pointers on the handle's GPU for labels, centers and found.
 */
int ctws_region_centers(ctws_handle* h, const uint64_t* labels, int64_t n_labels, int64_t k, const uint64_t* ids,
                        const int64_t* offsets, const int64_t* shapes, const int64_t* pitches,
                        const double resolution[3], int64_t* centers, uint8_t* found);
int ctws_region_centers_device(ctws_handle* h, const uint64_t* labels, int64_t n_labels, int64_t k,
                               const uint64_t* ids, const int64_t* offsets, const int64_t* shapes,
                               const int64_t* pitches, const double resolution[3], int64_t* centers,
                               uint8_t* found);

/*
 * ImageFilter (features/image_filter.py:105-115): vigra's Gaussian filters of one block, restated
 * (vigra is not available, parity at its boundary is unpinned).
 *
 * ctws_filter_taps: host code, no handle.  The 2 r + 1 taps for the offsets -r .. r of the Gaussian
 *   (order 0: radius int(3 sigma + 0.5), at least 1, taps summing to 1) or of its first or second
 *   derivative (order n: radius max(1, int((3 + n / 2) sigma + 0.5)), raw(x) = -x e(x) or
 *   (x^2 / sigma^2 - 1) e(x) with e(x) = exp(-x^2 / (2 sigma^2)), minus the mean of the raw values,
 *   scaled so that sum_x k(x) (-x)^n / n! = 1).  *radius = r always; out may be NULL (the radius
 *   alone), else it holds 2 r + 1 doubles.  CTWS_EINVAL for sigma <= 0, NaN or an order outside 0..2.
 *
 * ctws_image_filter / _device: data = one block (nz, ny, nx), C order, of dtype CTWS_U8, CTWS_U16,
 *   CTWS_F32 or CTWS_F64; out = float32 of the same shape.
 *     f       = float32(data); with normalize: f -= min(f); m = max(f); f /= m when m > 0
 *             (vu.normalize, float32 arithmetic)
 *     conv    along one axis with taps k of radius r: out[i] = float32(sum over p = i - r .. i + r
 *             ascending of k[i - p] * double(in[reflect(p)])), reflect(p) = -p or 2 (L - 1) - p,
 *             multiply and add separate, float32 between the axes, axes in the order z, y, x
 *     filter_id 0 gaussianSmoothing: S S S (S: order 0 along an axis, sigma[axis])
 *             1 gaussianGradientMagnitude: g_z = S_x S_y D_z, g_y = S_x D_y S_z, g_x = D_x S_y S_z
 *               (D: order 1); out = sqrtf((g_z g_z + g_y g_y) + g_x g_x) in float32, the square
 *               root correctly rounded
 *             2 laplacianOfGaussian: the same with the order-2 taps; out = (l_z + l_y) + l_x
 *     apply_in_2d: every z slice on its own -- the y and x passes alone, two components;
 *             sigma[0] is not read
 *   CTWS_EINVAL when an axis holds fewer voxels than a radius + 1 along it (the message names the
 *   axis and the radius; vigra refuses such a line), CTWS_EUNSUPPORTED for a radius above 48 or
 *   2^31 or more voxels.  Scratch of the handle: 8 (smoothing) or 20 bytes per voxel.  No
 *   floating-point atomics: the result depends on the inputs alone, and host and device pointers
 *   give the same bits.  ctws_last_timings reports if_minmax, if_first, if_y, if_x.  Host pointers
 *   are staged through HBM; _device takes device pointers on the handle's GPU for data and out.
 */
int ctws_filter_taps(double sigma, int order, double* out, int* radius);
int ctws_image_filter(ctws_handle* h, const void* data, int dtype, int64_t nz, int64_t ny, int64_t nx, int filter_id,
                      const double sigma[3], int apply_in_2d, int normalize, float* out);
int ctws_image_filter_device(ctws_handle* h, const void* data, int dtype, int64_t nz, int64_t ny, int64_t nx,
                             int filter_id, const double sigma[3], int apply_in_2d, int normalize, float* out);

/*
 * EdgeFeaturesWorkflow (features/features_workflow.py:14-66), BlockEdgeFeatures: the boundary-map
 * statistics of the edges of one block (block_edge_features.py:113-132,
 * `ndist.extractBlockFeaturesFromBoundaryMaps_*`, restated: DESIGN.md section 3.5).
 *
 * ctws_edge_features_block / _device: labels (uint64) and data (data_dtype CTWS_F32 or CTWS_U8;
 *   uint8 values are taken as float32(v) / float32(255)) on the block's extended box (nz, ny, nx),
 *   C order; (cz, cy, cx) <= (nz, ny, nx) is the extent of the core box [block.begin, block.end).
 *   nodes (n_nodes, ascending) and edges (n_edges x 2, sorted) are the block's sub-graph as
 *   ctws_rag_block gives it, ignore_label its `ignoreLabel`.
 *     pairs   every face-adjacent voxel pair (p, p + e_axis) with p in the core box, p + e_axis in
 *             the extended box and different ids -- neither 0 when ignore_label is set.  A pair
 *             wholly in the upper halo planes belongs to the neighbouring block: every pair of a
 *             volume is owned by exactly one block.
 *     samples each pair gives its edge both voxel values; the n = 2 * count samples of an edge are
 *             taken as float64 and sorted ascending into s
 *     out     n_edges x 10 float64, a row per edge in the order of edges:
 *             [mean, variance, min, q10, q25, q50, q75, q90, max, count] with mean = sum(s) / n,
 *             variance = sum((s - mean)^2) / n, quantile q = s[l] + (pos - l) (s[h] - s[l]) for
 *             pos = q (n - 1), l = floor(pos), h = min(l + 1, n - 1), count = the pairs.  An edge
 *             without an owned pair gets ten zeros.
 *   *n_missing (may be NULL) = the owned pairs whose edge is not in the table, as ctws_lookup_u64
 *   reports its misses; they contribute nothing.  n_edges == 0 returns at once (no launch, nothing
 *   counted).  CTWS_EINVAL when an edge has an endpoint that is no node or the edges are not
 *   sorted and unique.  Any finite value is legal, NaN is not supported.  The rows depend on the
 *   inputs alone (no floating-point atomics: repeated calls agree bit for bit).  Fewer than 2^31
 *   voxels and samples, 2^32 nodes and edges per block.  Host pointers are staged through HBM;
 *   _device takes device pointers on the handle's GPU for labels, data, nodes, edges and out.
 */
int ctws_edge_features_block(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype, int64_t nz,
                             int64_t ny, int64_t nx, int64_t cz, int64_t cy, int64_t cx, int ignore_label,
                             const uint64_t* nodes, int64_t n_nodes, const uint64_t* edges, int64_t n_edges,
                             double* out, int64_t* n_missing);
int ctws_edge_features_block_device(ctws_handle* h, const uint64_t* labels, const void* data, int data_dtype,
                                    int64_t nz, int64_t ny, int64_t nx, int64_t cz, int64_t cy, int64_t cx,
                                    int ignore_label, const uint64_t* nodes, int64_t n_nodes, const uint64_t* edges,
                                    int64_t n_edges, double* out, int64_t* n_missing);

/*
 * LiftedFeaturesFromNodeLabelsWorkflow (lifted_features/lifted_feature_workflow.py:80-198),
 * SparseLiftedNeighborhood: the lifted edges of a graph under a node labelling
 * (sparse_lifted_neighborhood.py:131-135, `ndist.computeLiftedNeighborhoodFromNodeLabels`, decided
 * here: DESIGN.md section 3.12).
 *
 * ctws_lifted_neighborhood / _device: edges (n_edges x 2) is the merged graph's edge table: u < v in
 *   every row, rows strictly ascending in (u, v), every id below n_nodes.  node_labels (n_nodes) is
 *   indexed by node id; a node whose label equals ignore_label is unlabelled.  depth >= 1.
 *   mode: CTWS_LIFTED_ALL, CTWS_LIFTED_SAME or CTWS_LIFTED_DIFFERENT.
 *     out   the pairs (u, v) with u < v, both labelled, hop distance 2 <= d(u, v) <= depth in the
 *           whole graph (paths may run through unlabelled nodes and through ids below u; pairs
 *           joined by an edge are not lifted), and labels that are equal (SAME), unequal
 *           (DIFFERENT) or either (ALL) as uint64.  Rows (k x 2), ascending in (u, v): the order of
 *           np.unique(axis=0).  A function of the inputs alone: repeated calls and host or device
 *           pointers give the same bytes.
 *   *n_out = k, always; CTWS_EINVAL when cap (in rows) is too small (nothing is written: retry with
 *   *n_out rows), when a row holds an id >= n_nodes, has u >= v or is not above its predecessor,
 *   for depth < 1 and for an unknown mode (the message says which).  n_edges == 0 and a labelling
 *   without a labelled node give 0 rows without a launch.  Limits, CTWS_EUNSUPPORTED otherwise:
 *   n_nodes < 2^32, n_edges < 2^31, k < 2^31.  Host pointers are staged through HBM; _device takes
 *   device pointers on the handle's GPU for edges, node_labels and out.
 */
#define CTWS_LIFTED_ALL       0
#define CTWS_LIFTED_SAME      1
#define CTWS_LIFTED_DIFFERENT 2
int ctws_lifted_neighborhood(ctws_handle* h, const uint64_t* edges, int64_t n_edges, const uint64_t* node_labels,
                             int64_t n_nodes, int depth, int mode, uint64_t ignore_label, uint64_t* out, int64_t cap,
                             int64_t* n_out);
int ctws_lifted_neighborhood_device(ctws_handle* h, const uint64_t* edges, int64_t n_edges,
                                    const uint64_t* node_labels, int64_t n_nodes, int depth, int mode,
                                    uint64_t ignore_label, uint64_t* out, int64_t cap, int64_t* n_out);
/* Two sizes of the search, for callers that size their tests by them (host code, no handle):
 * *first_capacity = the keys the first pass has room for with n_sources labelled nodes (a graph
 * with more lifted edges runs the search a second time at the counted size); *visited_capacity =
 * the nodes a wave's on-chip visited set takes (a source that reaches more goes on in a bitmap). */
int ctws_lifted_limits(int64_t n_sources, int64_t* first_capacity, int64_t* visited_capacity);

/*
 * ConnectedComponentsWorkflow and SizeFilterAndGraphWatershedWorkflow
 * (postprocess/postprocess_workflow.py:296-427): the two graph algorithms of the postprocessing over
 * the merged graph's edge table (graph_connected_components.py:104-121,
 * `ndist.connectedComponentsFromNodes` + `relabelConsecutive`; graph_watershed_assignments.py:152-178,
 * `nifty.graph.edgeWeightedWatershedsSegmentation`; decided here: DESIGN.md section 3.13).
 *
 * Both: edges (n_edges x 2) holds node ids below n_nodes (u != v; the order of the rows and of a
 * row's ends is free), the node array and out have n_nodes entries.  CTWS_EINVAL, with nothing
 * written to out, when a row holds an id >= n_nodes; CTWS_EUNSUPPORTED for n_nodes >= 2^32 or
 * n_edges >= 2^32.  n_edges == 0 launches no kernel over edges.  Results are functions of the inputs
 * alone: repeated calls and host or device pointers give the same bytes.  Host pointers are staged
 * through HBM; _device takes device pointers on the handle's GPU for every array.
 *
 * ctws_graph_components / _device: two nodes are joined when an edge connects them and both carry the
 *   same non-zero assignment.  out[i] = 0 where assignments[i] == 0, else 1 + the number of
 *   components whose smallest node id is below that of i's component.
 *
 * ctws_graph_watershed / _device: weights (n_edges) are float64, NaN is refused (CTWS_EINVAL), -0.0
 *   counts as 0.0; seeds[i] == 0 means unlabelled.  out is the result of the sequential flood: every
 *   edge between a labelled and an unlabelled node is queued, the edge with the smallest (weight,
 *   row index) is popped, and if exactly one end is unlabelled it takes the other's label and its
 *   edges to unlabelled nodes are queued.  Nodes that no seed reaches keep 0.  With relabel != 0 the
 *   result is renumbered by first appearance over the node index, from 1, zeros kept.  out must not
 *   be the seed array.  Computed in rounds whose number is bounded by the library (34, more than
 *   log2 of any admissible n_nodes); CTWS_EHIP if the bound is ever reached.
 */
int ctws_graph_components(ctws_handle* h, const uint64_t* edges, int64_t n_edges, const uint64_t* assignments,
                          int64_t n_nodes, uint64_t* out);
int ctws_graph_components_device(ctws_handle* h, const uint64_t* edges, int64_t n_edges, const uint64_t* assignments,
                                 int64_t n_nodes, uint64_t* out);
int ctws_graph_watershed(ctws_handle* h, const uint64_t* edges, const double* weights, int64_t n_edges,
                         const uint64_t* seeds, int64_t n_nodes, int relabel, uint64_t* out);
int ctws_graph_watershed_device(ctws_handle* h, const uint64_t* edges, const double* weights, int64_t n_edges,
                                const uint64_t* seeds, int64_t n_nodes, int relabel, uint64_t* out);

/*
 * ThresholdedComponentsWorkflow, BlockComponents (thresholded_components/block_components.py:
 * 143-230: `_cc_block` / `_cc_block_with_mask`, threshold + skimage.morphology.label) on the GPU.
 *
 * ctws_threshold_components: input = one float32 block (nz, ny, nx), C order; mask = uint8
 *   (nonzero = in mask) or NULL; normalize = 1 applies vu.normalize first (the unmasked,
 *   single-channel case); mode 0 'greater', 1 'less', 2 'equal' against threshold (compared as
 *   float32).  out (uint64, same shape) <- the 26-connected components of the members numbered
 *   1.. in order of first appearance in a C-order scan (skimage's numbering), 0 elsewhere;
 *   *n_labels = their number.  A block without members leaves out unwritten and *n_labels = 0
 *   (the reference returns 0 and writes nothing).  on_device: 1 device pointers, 0 host.
 *   Blocks of fewer than 2^32 - 1 voxels; a device input is 16-byte aligned when normalize = 1
 *   (CTWS_EINVAL otherwise; torch / hipMalloc allocations are).
 */
int ctws_threshold_components(ctws_handle* h, const float* input, const uint8_t* mask, int64_t nz, int64_t ny,
                              int64_t nx, int on_device, int mode, double threshold, int normalize, uint64_t* out,
                              int64_t* n_labels);
/*
 * ctws_threshold_components_ex: the same for any dtype of the dataset and with the Gaussian
 * prefilter (block_components.py:150-171 `_cc_block`, :198-222 `_cc_block_with_mask`):
 *   x = input (dtype: CTWS_U8 .. CTWS_U64); if normalize: x = vu.normalize(x) (float32);
 *   if sigma > 0: x = vu.normalize(gaussianSmoothing(float32(x), sigma)) (vigra: radius
 *   int(3 sigma + 0.5), reflect border, double accumulation, float32 between the axes);
 *   members = x `mode` threshold.  The comparison is numpy's for `x > python float`: float32
 *   against the threshold rounded to float32 when x is float32 (normalized, smoothed or a
 *   float32 dataset), float64 otherwise (float64 and integer datasets, NEP 50).  The caller
 *   passes normalize = 1 for an unmasked single-channel block (`_cc_block` normalizes the raw
 *   block) and for a masked block with sigma > 0 (`_cc_block_with_mask` normalizes before the
 *   filter).  A line shorter than radius + 1 along any axis is refused as vigra refuses it.
 */
int ctws_threshold_components_ex(ctws_handle* h, const void* input, int dtype, const uint8_t* mask, int64_t nz,
                                 int64_t ny, int64_t nx, int on_device, int mode, double threshold, int normalize,
                                 double sigma, uint64_t* out, int64_t* n_labels);
/*
 * MergeAssignments (thresholded_components/merge_assignments.py:125-130): out[i] = the
 * representative of label i after merging the (a, b) rows of pairs (n_pairs x 2, C order) into
 * nifty's boost_ufd(n) in row order -- boost::disjoint_sets union by rank (equal ranks: the first
 * root goes under the second).  Host code, no handle; CTWS_EINVAL for a label >= n.
 */
int ctws_ufd_find(int64_t n, const uint64_t* pairs, int64_t n_pairs, uint64_t* out);

/*
 * Test hooks (used by the parity tests, not by the task code): stop the pipeline after a
 * stage and read back one block's outer-shaped workspace array of the last batch.
 *   arrays: "fin" (float32 normalized input), "dt" (float32), "seedmap" (float32 smoothed
 *           dt), "hmap" (float32), "labels" (uint32; bit 31 = seed), "cls" (uint8)
 */
#define CTWS_STOP_NONE  0
#define CTWS_STOP_SEEDS 1  /* after seed labelling (labels = seeds)            */
#define CTWS_STOP_FLOOD 2  /* after the first flood (labels = watershed)        */
#define CTWS_STOP_WS    3  /* after the size filter + 2-D offsets + masking     */
int ctws_debug_set_stop(ctws_handle* h, int stage);
int ctws_debug_read(ctws_handle* h, const char* array, int block, void* dst, int64_t nbytes);
/* the EDT's correctly rounded sqrt of integers n0 .. n0 + count - 1 (< 2^24) into host dst */
int ctws_debug_sqrt_int(ctws_handle* h, uint32_t n0, uint32_t count, float* dst);

#ifdef __cplusplus
}
#endif

#endif /* CTWS_H */
