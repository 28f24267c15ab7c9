/*
 * bbme.h -- C-ABI of libbbme.so: MI355X-native block-matching motion estimation.
 *
 * Drop-in boundary for the hot path of ashish-nr/BlockBasedMotionEstimation:
 * MF::calcMotionBlockMatching() and everything it calls (pyramidal SAD spiral
 * full search + 8-neighbour MV regularisation), plus the Flow .flo codec and
 * the EPE evaluation.  The reference has no FFI; its boundary is the two C++
 * classes MF (motion_framework.h:9-54) and Flow (rw_flow.h:9-38).  Each entry
 * point below names the reference interface it replaces (paths relative to the
 * reference repository root).  All signatures are plain C: pointers and sizes,
 * no C++ or torch types.  Every function returns 0 (BBME_OK) or a negative
 * bbme_status; bbme_last_error() gives the message (thread-local).  Nothing in
 * this library ever calls exit() or abort().
 *
 * The compute path is HIP on gfx950 only.  There is no CPU fallback: entry
 * points that need the GPU fail with BBME_ERR_HIP when no device is usable.
 */
#ifndef BBME_H
#define BBME_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BBME_MAX_LEVELS 8
#define BBME_MAX_BATCH 64

typedef enum {
    BBME_OK = 0,
    BBME_ERR_INVALID = -1,      /* bad argument (null, non power-of-two block, sizes...)          */
    BBME_ERR_PADDING = -2,      /* "Could not find any multiples of the block size" (:21-26)       */
    BBME_ERR_ODD_PADDING = -3,  /* padded - original is odd: the reference mis-sizes the image     */
    BBME_ERR_DEGENERATE = -4,   /* < 2 blocks in a dimension at some level: reference reads OOB    */
    BBME_ERR_HIP = -5,          /* HIP runtime error / no gfx950 device                            */
    BBME_ERR_IO = -6,           /* .flo file errors (the reference prints and exit(1)s)            */
    BBME_ERR_STATE = -7,        /* call sequence error (e.g. estimate before frames were set)      */
    BBME_ERR_UNSUPPORTED = -8   /* legal in the reference but outside what the kernels implement   */
} bbme_status;

/* Parameters of MF::MF (motion_framework.h:12).  Index 0 = finest level,
 * num_levels-1 = coarsest (motion_framework.cpp:71-72,93-94,115).
 * search_size is the search-window SIDE LENGTH (range = (search_size-block_size)>>1). */
typedef struct {
    int num_levels;
    int block_size[BBME_MAX_LEVELS];
    int search_size[BBME_MAX_LEVELS];
} bbme_params;

typedef struct bbme_ctx bbme_ctx;

/* ---- no GPU needed ---------------------------------------------------------------- */

const char *bbme_version(void);
const char *bbme_last_error(void);

/* Padding search of MF::MF (motion_framework.cpp:14-54): public fields
 * padded_width/padded_height/padding_x/padding_y (motion_framework.h:16-19). */
int bbme_plan_padding(int width, int height, const bbme_params *params,
                      int *padded_width, int *padded_height, int *pad_x, int *pad_y);

/* Host-side pieces of MF::MF, exposed for callers that build planes themselves:
 * zero border (copyMakeBorder, :60-61) and one pyrDown step (:89-90). */
int bbme_pad_zero_host(const uint8_t *src, int width, int height, int pitch,
                       int pad_x, int pad_y, uint8_t *dst);
int bbme_pyr_down_host(const uint8_t *src, int src_width, int src_height, uint8_t *dst);
/* cv::resize(..., 4, 4, INTER_LINEAR) of main_class.cpp:32-33 (8-bit fixed point). */
int bbme_resize_x4_host(const uint8_t *src, int src_width, int src_height, uint8_t *dst);

/* Flow::ReadFlowFile (rw_flow.cpp:50-136).  *data is allocated by the library
 * (width*height*2 floats, u,v interleaved, row-major); release with bbme_free. */
int bbme_flo_read(const char *filename, int *width, int *height, float **data);
/* Flow::WriteFlowFile (rw_flow.cpp:139-200). */
int bbme_flo_write(const char *filename, int width, int height, const float *data);
/* Flow::WriteFlowFile on a worker thread (the reference's writer, rw_flow.cpp:139-200, has no caller and
 * is synchronous): submit hands over `height` rows of `width` (u, v) pairs starting at `data`, consecutive rows
 * `pitch_pixels` pixels apart -- e.g. the unpadded window of the padded field bbme_get_flow_host left in pinned memory:
 * data = flow + 2 * (pad_y * padded_width + pad_x), pitch_pixels = padded_width (main_class.cpp:63-70) -- and returns at
 * once; a writer with one worker writes the files in submission order, byte for byte what bbme_flo_write produces.  The
 * memory must stay untouched until a wait that covers the job returns; waits also report the first I/O error since the
 * last one.
 * bbme_flo_writer_create_pool: `workers` threads, one file each at a time -- files are independent, and one 66 MB file is
 * bound by the kernel's write path (three writers in flight write a 4K sequence twice as fast as
 * one); files then finish in any order.  Every submitted job has a ticket, 1, 2, ... in submission order:
 * bbme_flo_writer_ticket gives the last one handed out, bbme_flo_writer_wait_ticket returns once every job up to that
 * ticket is on disk (bbme_flo_writer_wait: every job submitted so far) -- what a pipeline needs that re-uses a staging
 * buffer round by round (csrc/seq_schedule.hpp: only round k - 2 has to be on disk before round k's download). */
typedef struct bbme_flo_writer bbme_flo_writer;
int bbme_flo_writer_create(bbme_flo_writer **out);
int bbme_flo_writer_create_pool(int workers, bbme_flo_writer **out);
int bbme_flo_writer_ticket(bbme_flo_writer *w, unsigned long long *ticket);
int bbme_flo_writer_wait_ticket(bbme_flo_writer *w, unsigned long long ticket);
int bbme_flo_writer_submit(bbme_flo_writer *w, const char *filename, int width, int height, const float *data,
                           int pitch_pixels);
/* The same file from the compact result (bbme_get_cells_host: one int16 (dx, dy) pair per 2x2 pixels of the padded level-0
 * field, cell_rows x cell_cols): copy_to_all_pixels (motion_framework.cpp:815-826), the padding strip (main_class.cpp:63-70)
 * and WriteFlowFile's rows fused on the worker, which expands and writes bands of rows with a few helper threads
 * (BBME_WRITER_THREADS, default 2; the kernel's write path is the bound).  Only 1/16 of the dense field crosses PCIe, and nobody holds 8 bytes per pixel in
 * memory.  Pixel (x, y) of the file = cell ((y + pad_y) / 2, (x + pad_x) / 2).  Byte for byte the file bbme_flo_write makes
 * of the dense field's window.  `cells` must stay untouched until bbme_flo_writer_wait returns. */
int bbme_flo_writer_submit_cells(bbme_flo_writer *w, const char *filename, int width, int height, const int16_t *cells,
                                 int cell_rows, int cell_cols, int pad_x, int pad_y);
int bbme_flo_writer_wait(bbme_flo_writer *w);
int bbme_flo_writer_destroy(bbme_flo_writer *w);
/* Flow::CalculateMSE (rw_flow.cpp:309-332): mean end-point error over known GT pixels. */
int bbme_calculate_mse(const float *gtruth, const float *flow, int width, int height, double *out);
/* Flow::MotionToColor (rw_flow.cpp:202-249, with computeColor :251-275 and makecolorwheel :277-300):
 * Middlebury colour coding of a flow field.  bgr = width*height*3 bytes, B,G,R per pixel as in the
 * reference's CV_8UC3 image; unknown pixels black; maxmotion > 0 overrides the normalising radius.
 * range (may be NULL) receives {max radius, min u, max u, min v, max v} of the known pixels, the
 * numbers the reference prints. */
int bbme_motion_to_color(const float *flow, int width, int height, float maxmotion, uint8_t *bgr, float *range);
/* What Flow::ShowImage (rw_flow.cpp:334-340) keeps on disk, as binary PPM (no PNG codec, no GUI here). */
int bbme_ppm_write_bgr(const char *filename, int width, int height, const uint8_t *bgr);
/* Binary PGM (P5, maxval 255), the grey sibling of bbme_ppm_write_bgr: "P5\n<width> <height>\n255\n", then `height` rows of
 * `width` bytes, consecutive rows `pitch` (>= width) bytes apart in `gray`. */
int bbme_pgm_write(const char *filename, int width, int height, int pitch, const uint8_t *gray);
/* main_class.cpp:58-70: strip padding, every 4th pixel, divide by 4. */
int bbme_subsample_div4(const float *flow_padded, int padded_width, int padded_height,
                        int pad_x, int pad_y, float *out, int out_width, int out_height);
void bbme_free(void *p);

/* Host tables of the search kernels, exposed for tests.  bbme_spiral_host: visiting order of
 * find_min_block_spiral (motion_framework.cpp:326-411), rank -> (dx, dy).  bbme_search_plan_host: the
 * work split of k_search_fast -- per round a code rounds[] = S | kind << 8 and 64 tasks (0xffffffff = idle lane):
 *   kind 0  strips: a lane takes column group g (candidate columns 4g .. 4g+3) and the S candidate rows from dy0;
 *           task = g | dy0 << 8;
 *   kind 1  the last candidate row of the tight plan (even ranges, block <= 16): the four lanes of a quad share one
 *           (group, row), a quarter of the block's rows each; task = g | dy << 8 | part << 16, part = 0..3;
 *   kind 2  the last candidate column of the tight plan (dx = +R), one candidate per lane; task = dy.
 * Together the tasks cover every candidate of the (2R+1)^2 square exactly once (kind 1: once per part). */
int bbme_spiral_host(int search_size, int block_size, int16_t *dx, int16_t *dy, int capacity, int *count);
int bbme_search_plan_host(int range, int block_size, uint32_t *rounds, int rounds_capacity, int *nrounds,
                          uint32_t *tasks /* rounds_capacity * 64 */, int *groups, int *pitch_dw);
/* the split used when `waves` (1 or 2) waves share a macroblock (levels with fewer blocks than the chip has SIMDs):
 * 64 * waves tasks per round, wave w takes tasks [64 w, 64 w + 64) of each */
int bbme_search_plan_host_waves(int range, int block_size, int waves, uint32_t *rounds, int rounds_capacity, int *nrounds,
                                uint32_t *tasks /* rounds_capacity * 64 * waves */, int *groups, int *pitch_dw);

/* ---- context: one per GPU stream (replaces an MF object) ---------------------------- */

/* Allocates every device buffer for a (width x height) frame pair: padded planes of
 * all levels, MV grids, work lists, the dense output.  device = HIP ordinal. */
int bbme_create(const bbme_params *params, int width, int height, int device, bbme_ctx **out);
/* A context for `pairs` (1..BBME_MAX_BATCH) independent frame pairs of one size: `pairs` MF objects behind one launch
 * sequence.  The reference holds all state of a pair in one MF object and carries nothing from pair to pair
 * (motion_framework.h:37-46), so the pairs of a sequence can be estimated side by side: every kernel of bbme_estimate then
 * works on all pairs at once (one more grid dimension), which is how a sequence keeps one GPU busy -- the regulariser of a
 * single pair is a chain of short dependent launches that leaves most of the chip idle, and the device dispatches dependent
 * kernels of many streams no faster than one per few microseconds.  Each pair's field is bit for bit what a context of its
 * own would produce.  Entry points without a pair index address pair 0. */
int bbme_create_batch(const bbme_params *params, int width, int height, int device, int pairs, bbme_ctx **out);
int bbme_batch_size(const bbme_ctx *ctx, int *pairs);
int bbme_destroy(bbme_ctx *ctx);
/* hipStream_t to run on (default: a stream the ctx creates).  Pass the raw handle. */
int bbme_set_stream(bbme_ctx *ctx, void *hip_stream);
/* The raw hipStream_t the context enqueues on (to order other work, e.g. a collective, behind bbme_estimate). */
int bbme_get_stream(bbme_ctx *ctx, void **hip_stream);
int bbme_get_geometry(const bbme_ctx *ctx, int *padded_width, int *padded_height,
                      int *pad_x, int *pad_y);
int bbme_level_geometry(const bbme_ctx *ctx, int level, int *width, int *height,
                        int *block_size, int *search_size);

/* ---- inputs ------------------------------------------------------------------------- */

/* MF::MF(image1, image2, ...) (motion_framework.cpp:4-111) for host images: uploads the two frames as they are and runs
 * the zero border (:57-61) and the pyrDown cascade (:86-106) as HIP kernels on the ctx stream, exactly as
 * bbme_set_frames_device does; returns when the upload has completed (the caller may re-use its buffers). */
int bbme_set_frames_host(bbme_ctx *ctx, const uint8_t *image1, const uint8_t *image2, int pitch);
int bbme_set_frames_host_pair(bbme_ctx *ctx, int pair, const uint8_t *image1, const uint8_t *image2, int pitch);
/* The same without the host wait: upload, border and pyramid are only enqueued on the ctx stream (truly asynchronous when
 * the source buffers are pinned: hipHostMalloc / hipHostRegister).  The buffers must stay untouched until the ctx stream
 * has passed this point (bbme_synchronize, or an event the caller records on bbme_get_stream's stream). */
int bbme_set_frames_host_async(bbme_ctx *ctx, int pair, const uint8_t *image1, const uint8_t *image2, int pitch);
/* Same constructor for frames already resident in HBM (unpadded, width x height):
 * zero padding and the whole pyrDown cascade run as HIP kernels on the ctx stream. */
int bbme_set_frames_device(bbme_ctx *ctx, const uint8_t *d_image1, const uint8_t *d_image2, int pitch);
int bbme_set_frames_device_pair(bbme_ctx *ctx, int pair, const uint8_t *d_image1, const uint8_t *d_image2, int pitch);
/* The reference's pipeline up-samples both frames x4 before MF::MF (main_class.cpp:32-33, cv::resize INTER_LINEAR).  These
 * setters take the ORIGINAL frames, (width / 4) x (height / 4) for a context created at the up-sampled width x height,
 * rows `pitch` bytes apart, and run the up-sampling fused with the zero border as one HIP kernel that writes every byte of
 * the level-0 planes, then the pyrDown cascade: planes byte for byte those of bbme_set_frames_host on
 * bbme_resize_x4_host's output, with a sixteenth of the bytes crossing PCIe.  BBME_ERR_INVALID when the context's width or
 * height is not a multiple of 4 or pitch < width / 4.  Otherwise as their plain counterparts: the host setter returns once
 * the upload has completed, the _async one only enqueues it (same buffer rules as bbme_set_frames_host_async), the device
 * setter reads HBM on the ctx stream. */
int bbme_set_frames_host_x4(bbme_ctx *ctx, int pair, const uint8_t *image1, const uint8_t *image2, int pitch);
int bbme_set_frames_host_x4_async(bbme_ctx *ctx, int pair, const uint8_t *image1, const uint8_t *image2, int pitch);
int bbme_set_frames_device_x4(bbme_ctx *ctx, int pair, const uint8_t *d_image1, const uint8_t *d_image2, int pitch);
/* A CHAIN context: `pairs` (1..BBME_MAX_BATCH) CONSECUTIVE pairs of a video over pairs + 1 frame slots, pair p = (slot p,
 * slot p + 1).  A video f0, f1, ... has the pairs (f0, f1), (f1, f2), ...: every inner frame is image 2 of one pair and image 1
 * of the next, and a batched context uploads it, pads it and runs it through the pyrDown cascade twice.  Every context keeps a
 * level's planes one plane stride apart in one allocation, image1 = its start; a batched context holds its pairs' image-1 planes
 * and, behind them, their image-2 planes, a chain context holds pairs + 1 planes with image2 = one stride further, so a frame
 * is set once and pair p reads slots p and p + 1 -- the kernels of bbme_estimate address pairs by that stride anyway and are
 * untouched.  Validation, errors and everything not named below (streams, modes, speculation / relaxation switches, *_pair
 * getters, bbme_subsampled_flow_device, bbme_compensation_error, the knobs) as bbme_create_batch with `pairs` pairs;
 * bbme_batch_size reports `pairs`.  A chain of one pair counts as a single-pair context (bbme_level_planes_device returns slot 0
 * and slot 1).  bbme_chain_frames: pairs + 1 for a chain context, 0 for any other.
 * bbme_set_chain_frames_*: slots first .. first + count - 1 from `count` frames, frames[i] (a HOST array of pointers in every
 * variant) pointing to host memory (_host, _host_async) or HBM (_device), rows `pitch` bytes apart.  scale 1: frames of the
 * context's size; scale 4: original frames of a quarter of the size, up-sampled as bbme_set_frames_*_x4 do.  A slot's planes are
 * byte for byte what bbme_set_frames_* / bbme_set_frames_*_x4 make of that frame.  The whole run is prepared by one launch per
 * level (border or up-sampling, then one pyrDown per level, the frame being a grid dimension) whatever `count` is.  _host
 * returns once the uploads have completed, _host_async only enqueues (buffer rules of bbme_set_frames_host_async), _device reads
 * HBM on the ctx stream (bbme_wait_for_stream orders it behind a producer).
 * bbme_chain_advance: enqueues, on the ctx stream and without a host wait, the copy of slot `pairs` (all levels, one launch) to
 * slot 0 -- the roll from one round of a video to the next; nothing is re-computed or re-uploaded.  Afterwards slot 0 is as set
 * as slot `pairs` was (set, in any sensible sequence) and slots 1 .. pairs are unset.  Results of the last estimate (flow,
 * cells, grids) stay readable.
 * State: while any slot is unset, every call that reads planes -- bbme_estimate, bbme_stage_search, bbme_stage_regularize, the
 * motion-compensation calls -- returns BBME_ERR_STATE.  Every frame setter and the roll reset the SAD memo.  The pair setters
 * (bbme_set_frames_*) return BBME_ERR_UNSUPPORTED on a chain context, the chain calls BBME_ERR_UNSUPPORTED on any other;
 * BBME_ERR_INVALID for first / count outside the slots, a null table or entry, pitch < width / scale, scale not 1 or 4, or
 * scale 4 on a context whose width or height is not a multiple of 4.
 * bbme_get_chain_plane_host: the padded plane of one slot (0 .. pairs) at one level, level width x level height bytes, as it
 * stands when the ctx stream reaches the call (set or not); returns after the copy.  For inspection: a chain of more than one
 * pair has no other plane getter (bbme_get_level_planes_host addresses one pair).  BBME_ERR_INVALID for a slot or level outside
 * the context or a null output. */
int bbme_create_chain(const bbme_params *params, int width, int height, int device, int pairs, bbme_ctx **out);
int bbme_chain_frames(const bbme_ctx *ctx, int *frames);
int bbme_set_chain_frames_host(bbme_ctx *ctx, int first, int count, const uint8_t *const *frames, int pitch, int scale);
int bbme_set_chain_frames_host_async(bbme_ctx *ctx, int first, int count, const uint8_t *const *frames, int pitch, int scale);
int bbme_set_chain_frames_device(bbme_ctx *ctx, int first, int count, const uint8_t *const *d_frames, int pitch, int scale);
int bbme_chain_advance(bbme_ctx *ctx);
int bbme_get_chain_plane_host(bbme_ctx *ctx, int level, int slot, uint8_t *image);
/* Which of the reference's two block searches MF::calcLevelBM calls (motion_framework.cpp:235-236): the spiral full
 * search find_min_block_spiral (:296-422, the live one: ties go to the candidate visited first on the spiral; a
 * prediction outside the image gives a zero MV) or the raster full search find_min_block (:246-294, commented out in the
 * reference: window clamped to the image, ties go to the candidate closer (L1) to the block's own position, then to the
 * first in raster order; a window entirely outside the image leaves the prediction as the result).  Default: spiral. */
enum { BBME_SEARCH_SPIRAL = 0, BBME_SEARCH_RASTER = 1 };
int bbme_set_search_mode(bbme_ctx *ctx, int mode);
/* BBME_REG_EXACT (default): every sweep leaves exactly the field of the reference's in-place raster sweep
 * (regularize_MVs writes each winner straight back, :616, and later blocks of the same sweep read it, :441-449).
 * BBME_REG_JACOBI: opt-in fast mode, NOT the reference's result -- every block of a sweep is evaluated against the field
 * as the previous sweep left it (one fully parallel pass per sweep, no dependent chains).  Same candidates, energies and
 * tie rules per block; the fields differ where a sweep's changes would have propagated within the sweep.  bench.py
 * reports its speed and its end-point error beside the exact mode's, never as `value`. */
enum { BBME_REG_EXACT = 0, BBME_REG_JACOBI = 1 };
int bbme_set_regularizer_mode(bbme_ctx *ctx, int mode);
/* Scheduling option (default on; BBME_SPECULATE=0 turns the default off): bbme_estimate starts the search of every level
 * but the coarsest on a second stream beside the coarser level's late regulariser sweeps, every block predicting from that
 * level's newest complete grid when the block starts, and afterwards searches again the blocks whose prediction those sweeps changed.  Same field, bit for bit;
 * shorter single pairs (the late sweeps leave most of the chip idle).  Turn it off when several contexts keep the chip
 * busy anyway (sequences with pairs in flight). */
int bbme_set_speculation(bbme_ctx *ctx, int enabled);
/* Scheduling option (default on): the relaxation launch (k_reg_iter) in front of the solver on large grids of small blocks takes
 * the heavy first generations of a sweep off the solver's latency-bound waves at the price of chip-wide work.  Same field,
 * bit for bit.  Turn it off, like the speculation, when several contexts keep the chip busy (8 pairs in flight at 4K:
 * 31.6 -> 33.2 Mblocks/s). */
int bbme_set_relaxation(bbme_ctx *ctx, int enabled);
/* Orders the ctx stream behind everything enqueued so far on another HIP stream of the same device (NULL = the default
 * stream): call it before bbme_set_frames_device when the frames were produced by asynchronous work on that stream.
 * Without it the caller must have synchronised the producer itself. */
int bbme_wait_for_stream(bbme_ctx *ctx, void *producer_stream);
/* Direct access to the ctx-owned padded planes of a level (device pointers, pitch ==
 * level width) so a caller can fill or inspect them in place.
 * IN-PLACE REFILL RULE.  The library is not told when planes change behind these pointers, and the regulariser's SAD memo
 * holds sums taken from the planes it last saw.  After a refill, the next stage call at the level must be bbme_stage_search
 * or bbme_stage_set_mvs (both start the memo afresh); bbme_estimate always does.  Running bbme_stage_regularize straight
 * after a refill is not supported.
 * SINGLE-PAIR ENTRY POINTS.  The three plane calls below, bbme_calculate_mse_device, every bbme_stage_* call,
 * bbme_sweep_stats, bbme_last_sweep_passes and bbme_gather_cells (bbme_rccl.h) address one pair: on a batched context
 * (bbme_create_batch with pairs > 1) they return BBME_ERR_UNSUPPORTED instead of quietly working on pair 0.  A batch
 * is fed with bbme_set_frames_{host,device}_pair and read with the *_pair getters. */
int bbme_level_planes_device(bbme_ctx *ctx, int level, uint8_t **d_image1, uint8_t **d_image2);
/* Upload ready-made padded planes of one level (fixtures taken after the pyramid). */
int bbme_set_level_planes_host(bbme_ctx *ctx, int level, const uint8_t *image1, const uint8_t *image2);
int bbme_get_level_planes_host(bbme_ctx *ctx, int level, uint8_t *image1, uint8_t *image2);

/* ---- the hot path ------------------------------------------------------------------- */

/* MF::calcMotionBlockMatching() (motion_framework.cpp:113-219).  Enqueues the whole
 * pyramid (search + regularisation of every level + dense expansion) on the ctx
 * stream and returns without waiting; no host synchronisation inside. */
int bbme_estimate(bbme_ctx *ctx);
int bbme_synchronize(bbme_ctx *ctx);
/* The cv::Mat returned by calcMotionBlockMatching (:218): dense padded H0 x W0
 * float2 (u,v) = (dx,dy), device pointer, pitch == padded width. */
int bbme_flow_device(bbme_ctx *ctx, const float **d_flow);
int bbme_flow_device_pair(bbme_ctx *ctx, int pair, const float **d_flow);
/* Synchronises, then copies the dense padded field to the host. */
int bbme_get_flow_host(bbme_ctx *ctx, float *flow /* padded_h * padded_w * 2 */);
int bbme_get_flow_host_pair(bbme_ctx *ctx, int pair, float *flow);
/* Compact result: one int16 (dx,dy) pair per 2x2 cell of level 0 ((H0/2) x (W0/2)). */
int bbme_cells_device(bbme_ctx *ctx, const int16_t **d_cells);
int bbme_cells_device_pair(bbme_ctx *ctx, int pair, const int16_t **d_cells);
/* copy_to_all_pixels (:815-826) for a cell grid that lives anywhere in HBM (e.g. gathered from
 * another GPU): writes the dense padded H0 x W0 float2 field to d_flow, on the ctx stream. */
int bbme_expand_cells_device(bbme_ctx *ctx, const int16_t *d_cells, float *d_flow);
/* The same on a caller-supplied HIP stream (NULL = the ctx stream), e.g. the stream a gather completes on,
 * so that the expansion of one step's results overlaps the next step's estimate. */
int bbme_expand_cells_device_on(bbme_ctx *ctx, const int16_t *d_cells, float *d_flow, void *hip_stream);
int bbme_get_cells_host(bbme_ctx *ctx, int16_t *cells);
int bbme_get_cells_host_pair(bbme_ctx *ctx, int pair, int16_t *cells);
/* The driver's subsampling (main_class.cpp:58-70: strip the padding, every `scale`-th pixel, divide by `scale`) straight
 * from the 2x2-cell grid: a ceil(width / scale) x ceil(height / scale) float2 (u, v) field of the unpadded frame, pixel
 * (x, y) = cell((pad_y + scale y) / 2, (pad_x + scale x) / 2) / scale.  scale 4 is bit for bit bbme_subsample_div4 of the
 * dense field, scale 1 its unpadded window; nothing dense is written or downloaded.  BBME_ERR_INVALID for scale < 1,
 * BBME_ERR_STATE before level 0 has reached 2x2 blocks (as bbme_calculate_mse_device).
 * bbme_subsampled_flow_device: into d_out (rows out_pitch_pixels float2 apart) on hip_stream (NULL = the ctx stream; another
 * stream is first ordered behind the ctx stream); no host wait.
 * bbme_get_subsampled_flow_host: synchronises, then packed rows into `out`. */
int bbme_subsampled_flow_device(bbme_ctx *ctx, int pair, int scale, float *d_out, int out_pitch_pixels, void *hip_stream);
int bbme_get_subsampled_flow_host(bbme_ctx *ctx, int pair, int scale, float *out);
/* Flow::CalculateMSE (rw_flow.cpp:309-332) on the device, fused with the driver's subsampling
 * (main_class.cpp:58-70): mean end-point error between a ground-truth field in HBM (gt_width x gt_height,
 * u,v interleaved) and the context's current result taken at every `scale`-th pixel of the unpadded frame and
 * divided by `scale` (4 for the reference's pipeline, 1 for none).  Per-pixel arithmetic is the reference's
 * float expression; the double sum is taken in a different order, so it agrees with bbme_calculate_mse to
 * about 1e-12 relative, not bit for bit.  Synchronises the ctx stream. */
int bbme_calculate_mse_device(bbme_ctx *ctx, const float *d_gtruth, int gt_width, int gt_height, int scale, double *out);

/* Motion compensation: MF::draw_MVimage (motion_framework.cpp:887-905), which the reference calls -- commented out -- on the
 * coarsest level with that level's block size ("MC_imageL3", :160-163) and on level 0 with 2x2 blocks after the whole
 * pyramid ("MC_imageL1", :205, 213-216), and the residual statistics of its frame against image1.
 * For pair p, level l and block size b, the compensated plane MC is W_l x H_l (bbme_level_geometry) and is built from the
 * level's CURRENT MV grid (block size cur_block): after bbme_estimate every level holds its final 2x2 grid; after stage calls,
 * whatever they left.  b is a power of two in 1..B_l.  The b-block with origin (X, Y) = (bx b, by b) takes the MV (dx, dy)
 * of the grid entry that covers pixel (X, Y), grid[Y / cur_block][X / cur_block].  Its source is (sx, sy) = (X + dx, Y + dy):
 * if 0 <= sx <= W_l - b and 0 <= sy <= H_l - b, MC[Y + i][X + j] = image2_l[sy + i][sx + j] for 0 <= i, j < b; otherwise
 * the block is skipped and its pixels get `fill` (0..255; the reference leaves them uninitialised).
 * This is the reference's draw_MVimage wherever its level_flow holds MVs at the b-block origins: after a level's last
 * divide_blocks (every level after bbme_estimate) for any b, b = 1 being a dense backward warp of image2; after
 * bbme_stage_search(l) for b = B_l; after the sweeps at b' for b' <= b <= B_l.
 * Residual statistics over a window {x0, y0, w, h} of the level plane (NULL = the whole plane) against image1_l, four
 * words per pair: sse = sum (MC - image1)^2, sad = sum |MC - image1|, pixels = window pixels whose block was compensated,
 * skipped = window pixels whose block was skipped.  Skipped pixels count in neither sum, so nothing depends on `fill`;
 * all four are exact integers.
 * Errors: BBME_ERR_INVALID for a null context or pointer, a pair or level out of range, a block that is not a power of two
 * in 1..B_l, a fill outside 0..255, a window not inside the plane, out_pitch < W_l; BBME_ERR_STATE when the level has no
 * grid yet.  These calls work on batched contexts and change no context state (grids, SAD memo, flow, cells).
 * bbme_motion_compensate_device: MC of `pair` into d_out (rows out_pitch bytes apart) on hip_stream (NULL = the ctx stream;
 * another stream is first ordered behind the ctx stream, as in bbme_subsampled_flow_device); no host wait.
 * bbme_get_motion_compensated_host: synchronises, then the packed W_l x H_l plane into `out`.
 * bbme_compensation_error: the statistics of EVERY pair in one launch, stats[4 p + {0, 1, 2, 3}] = sse, sad, pixels,
 * skipped; synchronises (like bbme_calculate_mse_device). */
int bbme_motion_compensate_device(bbme_ctx *ctx, int pair, int level, int block, int fill, uint8_t *d_out, int out_pitch,
                                  void *hip_stream);
int bbme_get_motion_compensated_host(bbme_ctx *ctx, int pair, int level, int block, int fill, uint8_t *out);
int bbme_compensation_error(bbme_ctx *ctx, int level, int block, const int *window, unsigned long long *stats);
/* The same rule on the CPU, no GPU: `grid` holds int16 (dx, dy) pairs, ceil(height / grid_block) rows of
 * ceil(width / grid_block); planes and `out` are packed width x height.  image1 may be NULL (no statistics), out may be NULL
 * (statistics only); stats4 = {sse, sad, pixels, skipped} or NULL.  Blocks cut by the plane's edge keep the rule. */
int bbme_motion_compensate_host(const uint8_t *image1, const uint8_t *image2, int width, int height, const int16_t *grid,
                                int grid_block, int block, int fill, const int *window, uint8_t *out,
                                unsigned long long *stats4);

/* ---- direction, bidirectional estimate and forward-backward consistency ---------------------------------------------- */

/* DIRECTION.  A context has a direction, BBME_DIR_FORWARD (default) or BBME_DIR_BACKWARD.  In direction BACKWARD every call that
 * reads planes or produces or reads results -- bbme_estimate, the bbme_stage_* calls, the flow / cells / subsampled getters,
 * bbme_calculate_mse_device, the three motion-compensation calls -- behaves bit for bit as it would on a context of the same kind
 * in which every pair had been set with image 1 and image 2 exchanged.  (The reference's MF is one-way, MF::MF(image1, image2,
 * ...): the backward field is the reference's field of the exchanged pair.)  Setters and the plane accessors (bbme_set_frames_*,
 * bbme_set_chain_frames_*, bbme_chain_advance, bbme_level_planes_device, bbme_set/get_level_planes_host) keep their physical
 * meaning in both directions: "image1" is what was set as image 1.  Changing the direction moves no byte of any plane -- the
 * kernels get the two plane bases exchanged; on a chain context pair p then reads slot p + 1 as its image 1 and slot p as its
 * image 2.  It does make every level's grid "nothing yet" (as after bbme_create: the cells / subsampled getters and the
 * motion-compensation calls return BBME_ERR_STATE until the next estimate or stage call) and restarts the SAD memo, because the
 * grids and the memo describe the other problem; setting the direction it already has changes nothing.  Each direction keeps a
 * captured launch graph of its own, so alternating directions does not capture again.  Of the two, one carries the forked branch
 * of the speculative search (bbme_set_speculation): FORWARD's, or BACKWARD's while the context has no FORWARD graph -- the first
 * FORWARD estimate after BACKWARD-only use waits once for the stream and has BACKWARD captured again without the branch.  Scheduling
 * only; every field is the same.  (A second forked graph on one context replays 0.9 ms slower at 4K than the first, whichever
 * direction it is; BBME_SPECULATE_BOTH_GRAPHS=1 forks both.)  BBME_ERR_INVALID for another value. */
enum { BBME_DIR_FORWARD = 0, BBME_DIR_BACKWARD = 1 };
int bbme_set_direction(bbme_ctx *ctx, int dir);
int bbme_get_direction(const bbme_ctx *ctx, int *dir);
/* BIDIRECTIONAL ESTIMATE.  Enqueues, on the ctx stream and without a host wait, the backward estimate of every pair, a copy of
 * its final 2x2-cell grid into a buffer of the context's own (the BACKWARD CELLS: shape and type of bbme_cells_device_pair, one
 * grid per pair), then the forward estimate (on first use the two graphs are captured, see above: a context without a FORWARD
 * graph waits once for the stream in that call).  Leaves the direction FORWARD whatever it was.  Afterwards every existing getter
 * returns exactly what it returns after bbme_estimate in direction FORWARD, and the backward cells are readable
 * (bbme_expand_cells_device makes a dense field of them).  No frame is uploaded, padded, up-sampled or pyramided again for the
 * backward half, on a chain context either.  BBME_ERR_STATE without frames / with an unset chain slot, as bbme_estimate.
 * The pair of fields is VALID from this call until the next call that can change either of them: any frame setter,
 * bbme_chain_advance, bbme_set_level_planes_host, bbme_estimate, bbme_stage_search / _regularize / _set_mvs, or
 * bbme_set_direction to another direction.  While it is not valid, bbme_backward_cells_device_pair,
 * bbme_get_backward_cells_host_pair, bbme_get_consistency_host and bbme_consistency_stats return BBME_ERR_STATE.  The sticky
 * "sweep did not converge" flag (bbme_synchronize) covers both halves. */
int bbme_estimate_bidirectional(bbme_ctx *ctx);
int bbme_backward_cells_device_pair(bbme_ctx *ctx, int pair, const int16_t **d_cells);
/* Synchronises, then downloads; reports non-convergence like bbme_get_cells_host. */
int bbme_get_backward_cells_host_pair(bbme_ctx *ctx, int pair, int16_t *cells);
/* CONSISTENCY RULE (this project's own; the reference has no such check).  Inputs: two cell grids A and B of CH x CW int16
 * (dx, dy) pairs (CH = H0 / 2, CW = W0 / 2 of the padded level-0 plane), a tolerance tol >= 0.  For cell (cx, cy) with
 * (dx, dy) = A[cy][cx]:
 *   target pixel (tx, ty) = (2 cx + dx, 2 cy + dy), in 32-bit integers;
 *   tx < 0, ty < 0, tx >= 2 CW or ty >= 2 CH: class BBME_FB_OUTSIDE, discrepancy not defined;
 *   otherwise (ex, ey) = B[ty >> 1][tx >> 1], d = |dx + ex| + |dy + ey| (up to 131 070), and the class is BBME_FB_CONSISTENT
 *   if d <= tol, else BBME_FB_INCONSISTENT.
 * The mask is one byte per cell holding the class.  The statistics over a window {cx0, cy0, cw, ch} IN CELLS (NULL = all
 * cells) are four exact 64-bit integers: cells of class 0, of class 1, of class 2, and the sum of d over the window's cells of
 * class 0 or 1.  which = BBME_DIR_FORWARD: A = forward cells, B = backward cells (the mask lives on frame 1: where it is 1,
 * frame 1's content has no agreeing partner in frame 2); which = BBME_DIR_BACKWARD the other way round (mask on frame 2).
 * Errors: BBME_ERR_INVALID for a null context or required pointer, a pair out of range, `which` not 0 or 1, tol < 0, a window
 * with a negative origin, an empty side or reaching outside CW x CH, mask_pitch < CW; BBME_ERR_STATE for the context-level calls
 * without a valid pair of fields.  None of these calls changes context state (grids, memo, flow, cells, backward cells); their
 * scratch buffers are independent of the other getters'.  All work on single, batched and chain contexts.
 * bbme_cells_consistency_device: the rule on ANY two cell grids in HBM of this context's cell geometry (bbme_cells_device_pair
 * and bbme_backward_cells_device_pair, or grids gathered from another GPU); d_mask (rows mask_pitch bytes apart) and d_stats4
 * each may be null, not both; on hip_stream (NULL = the ctx stream; another stream is first ordered behind it, as
 * bbme_motion_compensate_device); no host wait; needs no valid pair of fields.  Launches with d_stats4 share one scratch buffer
 * per context: the caller orders those it issues on different streams.
 * bbme_get_consistency_host: the context's own two fields of `pair`; synchronises; packed CH x CW bytes.
 * bbme_consistency_stats: EVERY pair in one launch, stats[4 p + k]; synchronises (like bbme_compensation_error).
 * bbme_cells_consistency_host: the same rule on the CPU, no GPU, on packed cells_h x cells_w grids; mask (packed) and stats4
 * each may be NULL, not both. */
enum { BBME_FB_CONSISTENT = 0, BBME_FB_INCONSISTENT = 1, BBME_FB_OUTSIDE = 2 };
int bbme_cells_consistency_device(bbme_ctx *ctx, const int16_t *d_a, const int16_t *d_b, int tol, const int *window,
                                  uint8_t *d_mask, int mask_pitch, unsigned long long *d_stats4, void *hip_stream);
int bbme_get_consistency_host(bbme_ctx *ctx, int pair, int which, int tol, uint8_t *mask);
int bbme_consistency_stats(bbme_ctx *ctx, int which, int tol, const int *window, unsigned long long *stats);
int bbme_cells_consistency_host(const int16_t *a, const int16_t *b, int cells_w, int cells_h, int tol, const int *window,
                                uint8_t *mask, unsigned long long *stats4);

/* COLOUR RULE: Flow::MotionToColor (rw_flow.cpp:202-249, with computeColor :251-275) of the field the driver makes of the result
 * (main_class.cpp:58-75: strip the padding, every scale-th pixel, divide by scale, MotionToColor), straight from a 2x2-cell grid.
 * Input: a cell grid, int16 (dx, dy) per cell, CH x CW = (padded_h / 2) x (padded_w / 2); a subsampling step scale >= 1; maxmotion.
 * Output: the ow x oh B,G,R image, ow = ceil(W / scale), oh = ceil(H / scale) of the unpadded W x H frame, and
 * range[5] = {max radius, min u, max u, min v, max v}.
 * Pixel (x, y) takes (dx, dy) = cell[(pad_y + scale y) >> 1][(pad_x + scale x) >> 1], u = (float)dx / (float)scale, v likewise:
 * exactly the field of bbme_subsampled_flow_device / bbme_get_subsampled_flow_host.
 * Range pass, as MotionToColor's (:205-221): max u, max v, min u, min v start from the reference's sentinels -999, -999, 999, 999
 * and the max radius from -1, and every pixel is folded in with rad = sqrtf(u * u + v * v) in float (no FMA).  The sentinels
 * matter: a four-level field of search range 127 can exceed 999, and a minimum then stays 999 as bbme_motion_to_color reports it.
 * maxrad = maxmotion if maxmotion > 0, else the max radius; a maxrad of 0 becomes 1 (:225-229).  (No cell is "unknown".)
 * Colour pass: computeColor of (fx, fy) = (u / maxrad, v / maxrad) in the reference's float / double expression order, as
 * compute_color of csrc/bbme_host.cpp states it (rad = sqrtf(fx * fx + fy * fy); fk = (a + 1.0f) / 2.0f * 54.0f; k0 = (int)fk;
 * k1 = (k0 + 1) % 55; f = fk - k0; per channel col = (1 - f) * col0 + f * col1 with col_i = wheel / 255.0f, then
 * 1 - rad * (1 - col) for rad <= 1, else (float)(col * .75); byte = (int)(255.0 * col)), nothing contracted into an FMA --
 * with ONE deliberate difference, the hue angle.  The reference's atan2(-fy, -fx) on floats is the platform's float atan2f,
 * which need not be correctly rounded (glibc 2.35's differs from the rounded double result in the last bit on about 16 % of
 * arguments) and which a GPU cannot reproduce version by version.  The rule here is
 *     A = (float)atan2((double)-fy, (double)-fx),  a = (float)((double)A / 3.14159265358979323846).
 * Signs of zero survive: dy = 0 gives -fy = -0.0f, and atan2(-0.0, negative) is -pi, not +pi.
 * What that costs: against bbme_motion_to_color of the same field the range is identical and the image agrees except where an
 * angle one float ulp apart moves a channel across an integer boundary -- no channel by more than 1 level, and on the integer
 * vectors |d| <= 64 at scale 1 and 4 no channel at all (tests/test_flow_color_cpu.py holds it to at most 1e-4 of the channels).
 * All entry points: BBME_ERR_INVALID for a null context or pointer, a pair out of range, `which` not BBME_DIR_FORWARD /
 * BBME_DIR_BACKWARD, scale < 1, a pitch below 3 ow.  They work on single, batched and chain contexts and on contexts made for
 * up-sampled frames, and change no context state (grids, flow, cells, backward cells, SAD memo, captured graphs); their scratch
 * buffers are the context's own and independent of the other getters'.  When maxmotion > 0 and no range is asked for, the range
 * pass is not run.
 * bbme_cells_color_device: the rule on ANY cell grid in HBM of this context's cell geometry; needs no estimate.  d_bgr (rows
 * out_pitch_bytes apart; any alignment) and d_range (five floats) each may be null, not both; on hip_stream (NULL = the ctx
 * stream; another stream is first ordered behind it); no host wait.  The two passes meet in HBM, not on the host.  Calls
 * share one scratch slot per context: the caller orders those it issues on different streams.
 * bbme_flow_color_device: the same on the context's own cells of `pair` (scratch slot: one per pair): which = BBME_DIR_FORWARD
 * the current level-0 cells (BBME_ERR_STATE before level 0 has reached 2x2 blocks, as bbme_subsampled_flow_device), which =
 * BBME_DIR_BACKWARD the cells kept by bbme_estimate_bidirectional (BBME_ERR_STATE without a valid pair of fields, as
 * bbme_backward_cells_device_pair).
 * bbme_get_flow_color_host: synchronises; packed rows of 3 ow bytes into bgr, the five floats into range5; each may be NULL,
 * not both.
 * bbme_flow_ranges: the five floats of EVERY pair from one launch, ranges[5 p + k]; synchronises.  (A video coloured with one
 * common maxmotion takes the largest ranges[5 p].)
 * bbme_cells_color_host: the same rule on the CPU, no GPU, on a packed cells_h x cells_w grid: the width x height frame at
 * (pad_x, pad_y) of the 2 cells_w x 2 cells_h plane (BBME_ERR_INVALID when it does not lie inside); bgr (packed) and range5
 * each may be NULL, not both. */
int bbme_cells_color_device(bbme_ctx *ctx, const int16_t *d_cells, int scale, float maxmotion, uint8_t *d_bgr, int out_pitch_bytes,
                            float *d_range, void *hip_stream);
int bbme_flow_color_device(bbme_ctx *ctx, int pair, int which, int scale, float maxmotion, uint8_t *d_bgr, int out_pitch_bytes,
                           float *d_range, void *hip_stream);
int bbme_get_flow_color_host(bbme_ctx *ctx, int pair, int which, int scale, float maxmotion, uint8_t *bgr, float *range5);
int bbme_flow_ranges(bbme_ctx *ctx, int which, int scale, float *ranges);
int bbme_cells_color_host(const int16_t *cells, int cells_w, int cells_h, int width, int height, int pad_x, int pad_y, int scale,
                          float maxmotion, uint8_t *bgr, float *range5);

/* INTERPOLATION RULE (this project's own; the reference has no interpolation): the frame at phase num / den between frame 1
 * (phase 0) and frame 2 (phase 1) of a pair, motion-compensated from both fields.  Inputs: the level-0 padded planes I1 and I2
 * (W0 x H0 bytes), the cell grid F on frame 1 (forward) and, optionally, the cell grid B on frame 2 (backward), CH x CW int16
 * (dx, dy) pairs each (CH = H0 / 2, CW = W0 / 2), and the phase, 2 <= den <= 256 and 0 < num < den.  All arithmetic is in 32-bit
 * integers; den / 2 is the integer half; floor_div rounds towards minus infinity.
 * Output cell (cx, cy) with origin (ox, oy) = (2 cx, 2 cy) has up to three hypotheses, in this order:
 *   k = 0: v = F[cy][cx];   k = 1: v = -B[cy][cx] (absent without B);   k = 2: v = (0, 0).
 * For a hypothesis v = (vx, vy): the shift s = (floor_div(num vx + den / 2, den), floor_div(num vy + den / 2, den)),
 * p1 = (ox, oy) - s and p2 = p1 + v (so p2 - p1 = v exactly).  It is valid when both 2x2 cells lie inside the plane,
 * 0 <= p1.x, p2.x <= W0 - 2 and 0 <= p1.y, p2.y <= H0 - 2 (k = 2 always is), and its cost is the sum over the four pixels of
 * |I1[p1 + (j, i)] - I2[p2 + (j, i)]|, 0..1020.  The valid hypothesis of the smallest cost is selected; of equal costs the earliest.
 * With its p1 and p2, out[oy + i][ox + j] = ((den - num) I1[p1 + (j, i)] + num I2[p2 + (j, i)] + den / 2) / den for 0 <= i, j < 2.
 * The selection map holds one byte k per cell.  The statistics over a window {cx0, cy0, cw, ch} IN CELLS (NULL = all cells) are
 * four exact 64-bit integers: cells that selected k = 0, k = 1, k = 2, and the sum of the selected costs.
 * One call makes `count` consecutive phases num0 .. num0 + count - 1 of one den in ONE launch (the phase is a grid dimension;
 * planes and grids come from L2 for all but the first): frame q at d_out + q out_stride, its map at d_sel + q sel_stride, its
 * statistics at d_stats4[4 q ..].  A context created for up-sampled frames (bbme_set_frames_*_x4) interpolates its 4x planes.
 * Errors: BBME_ERR_INVALID for a null context or required pointer, a pair out of range, den outside 2..256, num0 < 1, count < 1,
 * num0 + count > den, out_pitch < W0, sel_pitch < CW, a stride below one frame (out_pitch H0, sel_pitch CH) when count > 1, a
 * window as for the consistency rule, an odd width or height on the host call; BBME_ERR_STATE when frames are unset or a chain
 * slot is unset, and for the three context-level calls without a valid pair of fields (as the backward cells).  None of these
 * calls changes context state; their scratch buffers are independent of the other getters'.  All work on single, batched and
 * chain contexts; in direction BACKWARD the two planes exchange, as for every plane-reading call.
 * bbme_cells_interpolate_device: the context's planes of `pair` and ANY two grids in HBM of its cell geometry (d_bwd may be
 * null); d_out, d_sel and d_stats4 each may be null, not all three; on hip_stream (NULL = the ctx stream; another stream is
 * first ordered behind it); no host wait; needs no valid pair of fields.  Launches with d_stats4 share one scratch buffer per
 * context: the caller orders those it issues on different streams.
 * bbme_interpolate_device: the same on the context's own two fields, frames only.
 * bbme_get_interpolated_host: one phase of the context's own fields; synchronises; packed W0 x H0 bytes.
 * bbme_interpolation_stats: EVERY pair in one launch, stats[4 p + k]; synchronises (like bbme_consistency_stats).
 * bbme_interpolate_host: the same rule on the CPU, no GPU, on packed width x height planes (both even) and packed
 * (height / 2) x (width / 2) grids; out, sel (packed) and stats4 each may be NULL, not all three. */
int bbme_cells_interpolate_device(bbme_ctx *ctx, int pair, const int16_t *d_fwd, const int16_t *d_bwd, int num0, int count, int den,
                                  const int *window, uint8_t *d_out, int out_pitch, size_t out_stride, uint8_t *d_sel,
                                  int sel_pitch, size_t sel_stride, unsigned long long *d_stats4, void *hip_stream);
int bbme_interpolate_device(bbme_ctx *ctx, int pair, int num0, int count, int den, uint8_t *d_out, int out_pitch,
                            size_t out_stride, void *hip_stream);
int bbme_get_interpolated_host(bbme_ctx *ctx, int pair, int num, int den, uint8_t *out);
int bbme_interpolation_stats(bbme_ctx *ctx, int num, int den, const int *window, unsigned long long *stats);
int bbme_interpolate_host(const uint8_t *image1, const uint8_t *image2, int width, int height, const int16_t *fwd,
                          const int16_t *bwd, int num, int den, const int *window, uint8_t *out, uint8_t *sel,
                          unsigned long long *stats4);

/* ---- colour video: B,G,R frames in, motion-compensated B,G,R frames out ("bgr" in names; "color" means the flow colour coding) -- */

/* LUMA RULE (this project's own; the reference's driver reads its colour PNGs as grey, imread(path, 0), main_class.cpp:24-26, and
 * no bit-identity with any library's conversion is claimed).  A colour frame is H rows of W pixels of 3 bytes in B,G,R order (the
 * order of bbme_ppm_write_bgr's input), consecutive rows `pitch` >= 3 W bytes apart.  Its luma is
 *     Y = (1868 B + 9617 G + 4899 R + 8192) >> 14,   in 32-bit integers:
 * the BT.601 weights in 14 bits.  They sum to 16384, so B = G = R = g gives Y = g exactly, and Y <= 255 always.
 * bbme_bgr_to_gray_host: the rule on the CPU, no GPU; `gray` is packed width x height.
 * The *_bgr frame setters below are, plane by plane and bit for bit, the grey setter of the same name on that luma -- the level-0
 * planes are pad_zero(Y), deeper levels its pyrDown cascade -- from ONE kernel that converts and writes the zero border, and they
 * keep the colour: a context holds one packed (pitch 3 W) B,G,R copy per frame it holds (the two of every pair, or the slots of
 * a chain context: bbme_bgr_frames_device_pair tells where a pair's lie), in a COLOUR STORE allocated by the first colour setter.
 * Host setters upload straight into the store (the frame crosses PCIe once) and convert from there; device setters read the
 * caller's frames on the ctx stream and copy them into the store in the same pass.
 * A frame HAS COLOUR from a *_bgr setter until a grey setter of that frame (bbme_set_frames_*, the _x4 forms,
 * bbme_set_chain_frames_* on its slot, bbme_set_level_planes_host): the stored colour then is not what the luma plane was made
 * from, and the calls that read stored colour return BBME_ERR_STATE.  bbme_chain_advance moves the last slot's colour with its
 * planes.  (Planes refilled in place through bbme_level_planes_device are the caller's business, as for the SAD memo.)
 * Scale 1 only: there is no colour form of the x4 setters.  Bookkeeping (frames set, SAD memo, validity of the pair of fields),
 * waiting (_host returns after the upload, _host_async only enqueues, _device reads HBM on the ctx stream) and the pair / chain
 * refusals are the grey setters'; BBME_ERR_INVALID for a null pointer, a pair, first or count out of range, pitch < 3 W.
 * A caller's device frames must not overlap the colour store (the pointers bbme_bgr_frames_device_pair returns): the device
 * setters write the store in the pass that reads the frames.
 * bbme_bgr_frames_device_pair: the stored frames of `pair` as set (image 1, image 2; physical in both directions), pitch 3 W;
 * BBME_ERR_STATE unless both have colour. */
int bbme_bgr_to_gray_host(const uint8_t *bgr, int width, int height, int pitch, uint8_t *gray);
int bbme_set_frames_host_bgr(bbme_ctx *ctx, int pair, const uint8_t *image1, const uint8_t *image2, int pitch);
int bbme_set_frames_host_bgr_async(bbme_ctx *ctx, int pair, const uint8_t *image1, const uint8_t *image2, int pitch);
int bbme_set_frames_device_bgr(bbme_ctx *ctx, int pair, const uint8_t *d_image1, const uint8_t *d_image2, int pitch);
int bbme_set_chain_frames_host_bgr(bbme_ctx *ctx, int first, int count, const uint8_t *const *frames, int pitch);
int bbme_set_chain_frames_host_bgr_async(bbme_ctx *ctx, int first, int count, const uint8_t *const *frames, int pitch);
int bbme_set_chain_frames_device_bgr(bbme_ctx *ctx, int first, int count, const uint8_t *const *d_frames, int pitch);
int bbme_bgr_frames_device_pair(bbme_ctx *ctx, int pair, const uint8_t **d_bgr1, const uint8_t **d_bgr2);

/* BGR INTERPOLATION RULE.  Inputs: those of the interpolation rule -- the level-0 padded LUMA planes I1, I2 (W0 x H0), the cell
 * grids F and, optionally, B, the phase num / den -- and the two colour frames C1, C2 (W x H pixels of B,G,R) whose lumas the
 * planes hold at (pad_x, pad_y): W0 = W + 2 pad_x, H0 = H + 2 pad_y.
 * Selection is EXACTLY the interpolation rule's, on the luma planes, in padded coordinates: hypotheses, their order, validity,
 * cost, ties, p1 and p2 are unchanged, so the selection map and the statistics of a colour frame are those
 * bbme_cells_interpolate_device returns; the colour calls make neither.
 * The output is the UNPADDED W x H B,G,R frame.  Output pixel (x, y) has the padded position (X, Y) = (x + pad_x, y + pad_y) and
 * belongs to cell (X >> 1, Y >> 1) at offset (j, i) = (X & 1, Y & 1).  With that cell's p1 and p2, for every channel c
 *     out[y][x][c] = ((den - num) C1[q1][c] + num C2[q2][c] + den / 2) / den,
 *     q1 = p1 + (j, i) - (pad_x, pad_y),  q2 = p2 + (j, i) - (pad_x, pad_y)   (frame coordinates),
 * where a q outside [0, W) x [0, H) reads 0 in every channel: the zero border the luma planes have.  pad_x and pad_y may be odd
 * (bbme_plan_padding only makes the padded size minus the frame's even): cells then straddle the frame's edge and only their pixels
 * inside the frame are written.  On frames with B = G = R every channel of the result is the unpadded window of the grey result.
 * `count` consecutive phases come from one launch, frame q at d_out + q out_stride, rows out_pitch bytes apart (any alignment).
 * Errors: BBME_ERR_INVALID as for the grey calls (null context or required pointer, pair, den, num0, count), and for
 * out_pitch < 3 W, bgr_pitch < 3 W, a stride below one frame (out_pitch H) when count > 1, exactly one of d_bgr1 / d_bgr2 null;
 * BBME_ERR_STATE when frames are unset, when stored colour is asked for and either frame of the pair has none, and for the two context-level calls
 * without a valid pair of fields.  None of these calls changes context state.  All work on single, batched and chain contexts; in
 * direction BACKWARD the two colour frames exchange together with the two planes (callers' frames too).
 * bbme_cells_interpolate_bgr_device: the context's planes of `pair`, ANY two grids in HBM of its cell geometry (d_bwd may be
 * null) and either the stored colour (d_bgr1 = d_bgr2 = null) or a caller's two frames in HBM, rows bgr_pitch bytes apart -- whose
 * lumas must be what the planes were made from for the result to mean anything; on hip_stream (NULL = the ctx stream; another
 * stream is first ordered behind it); no host wait; needs no valid pair of fields.
 * bbme_interpolate_bgr_device: the same on the context's own two fields and stored colour.
 * bbme_get_interpolated_bgr_host: one phase of those; synchronises; packed rows of 3 W bytes.
 * bbme_interpolate_bgr_host: the rule on the CPU, no GPU: packed padded_w x padded_h luma planes (both even), packed width x height
 * colour frames, packed (padded_h / 2) x (padded_w / 2) grids (bwd may be NULL), out packed 3 width x height; BBME_ERR_INVALID
 * unless padded_w = width + 2 pad_x and padded_h = height + 2 pad_y with pads >= 0. */
int bbme_cells_interpolate_bgr_device(bbme_ctx *ctx, int pair, const int16_t *d_fwd, const int16_t *d_bwd, const uint8_t *d_bgr1,
                                      const uint8_t *d_bgr2, int bgr_pitch, int num0, int count, int den, uint8_t *d_out,
                                      int out_pitch, size_t out_stride, void *hip_stream);
int bbme_interpolate_bgr_device(bbme_ctx *ctx, int pair, int num0, int count, int den, uint8_t *d_out, int out_pitch,
                                size_t out_stride, void *hip_stream);
int bbme_get_interpolated_bgr_host(bbme_ctx *ctx, int pair, int num, int den, uint8_t *out);
int bbme_interpolate_bgr_host(const uint8_t *luma1, const uint8_t *luma2, int padded_w, int padded_h, const uint8_t *bgr1,
                              const uint8_t *bgr2, int width, int height, int pad_x, int pad_y, const int16_t *fwd,
                              const int16_t *bwd, int num, int den, uint8_t *out);

/* ---- motion-compensated temporal denoising: a frame averaged with its two motion-aligned neighbours ---------------------- */

/* TEMPORAL FILTER RULE (this project's own; the reference has no temporal filter).  Inputs: the plane C of the frame to filter;
 * optionally the plane P of the previous frame with the cell grid GP on C that points into P; optionally the plane N of the next
 * frame with the cell grid GN on C that points into N; a strength thr, 1 <= thr <= 1021.  Planes are packed W0 x H0 bytes (the
 * level-0 padded geometry), grids CH x CW int16 (dx, dy) pairs, CH = H0 / 2, CW = W0 / 2.  A neighbour is PRESENT when its plane
 * and its grid are both given; at least one must be.  All arithmetic is in 32-bit integers; every division is the floor
 * division of non-negative numbers.
 * For output cell (cx, cy) with origin o = (2 cx, 2 cy) and each present neighbour X (P or N) with grid G:
 *   v = G[cy][cx], p = o + v;
 *   the neighbour is valid when 0 <= p.x <= W0 - 2 and 0 <= p.y <= H0 - 2;
 *   cost = sum over the four pixels 0 <= i, j < 2 of |C[o + (j, i)] - X[p + (j, i)]|, 0..1020;
 *   w = 8 (thr - cost) / thr if the neighbour is valid and cost < thr, else 0.
 * So w is in 0..8 and w = 8 only at cost 0; an absent neighbour has w = 0.  With S = 8 + wP + wN (8..24),
 *   out[o + (j, i)] = (8 C[o + (j, i)] + wP P[pP + (j, i)] + wN N[pN + (j, i)] + S / 2) / S    for 0 <= i, j < 2.
 * The weight map holds one byte per cell, wP | wN << 4.  The statistics over a window {cx0, cy0, cw, ch} IN CELLS (NULL = all
 * cells) are four exact 64-bit integers: cells with wP > 0, cells with wN > 0, the sum of wP + wN, and the sum over the window's
 * pixels of |out - C|.  The statistics and the map do not need the frame to be written.
 * On a context with its own fields (bbme_estimate_bidirectional) the grid into the previous frame is the BACKWARD cells of the
 * pair the frame is image 2 of, and the grid into the next frame the FORWARD cells of the pair it is image 1 of: both live on
 * the frame itself.  A context made for up-sampled frames filters its 4x planes; on a colour context the planes are the luma and
 * that is what these calls filter, exactly as on a grey context; the colour frames themselves are filtered by the BGR TEMPORAL
 * FILTER RULE below, which takes its weights from the colour frames and not from the luma (the table there says why).
 * Errors: BBME_ERR_INVALID for a null context or required pointer, pair / which / first / count out of range, thr outside
 * 1..1021, out_pitch < W0, weights_pitch < CW, out_stride below one frame (out_pitch H0) when count > 1, a window as for the
 * consistency rule, exactly one of a neighbour's plane and grid, no neighbour at all, a d_out of bbme_cells_temporal_filter_device
 * that overlaps one of its input planes, an odd width or height on the host call;
 * BBME_ERR_UNSUPPORTED for bbme_temporal_filter_chain_device on anything but a chain context; BBME_ERR_STATE for the four
 * context-level calls (bbme_temporal_filter_device, _chain_device, bbme_get_temporal_filtered_host, bbme_temporal_filter_stats)
 * without a valid pair of fields, exactly as bbme_backward_cells_device_pair -- hence they always run in direction FORWARD.
 * None of these calls changes context state (grids, memo, flow, cells, backward cells, captured graphs, colour store); their
 * scratch buffers are the context's own and independent of the other getters'.  Outputs must not overlap inputs.
 * bbme_temporal_filter_host: the rule on the CPU, no GPU, on packed width x height planes (both even) and packed
 * (height / 2) x (width / 2) grids; out, weights (packed) and stats4 each may be NULL, not all three.
 * bbme_cells_temporal_filter_device: ANY three packed planes and ANY two grids in HBM of the context's level-0 / cell geometry
 * (another context's, or a caller's copies); no frames set and no estimate needed; d_out (rows out_pitch bytes apart), d_weights
 * (rows weights_pitch apart) and d_stats4 each may be null, not all three; on hip_stream (NULL = the ctx stream; another stream is
 * first ordered behind it); no host wait.  Launches with d_stats4 share one scratch buffer per context: the caller orders those
 * it issues on different streams.
 * bbme_temporal_filter_device: frame `which` (0 = image 1, 1 = image 2) of `pair` from the context's own planes and fields.  On a
 * pair or batched context image 1 has only its next neighbour (image 2, forward cells) and image 2 only its previous one (image 1,
 * backward cells).  On a chain context the frame is slot pair + which and uses both neighbours where they exist: slot f - 1 with
 * the backward cells of pair f - 1, slot f + 1 with the forward cells of pair f; (p, 1) and (p + 1, 0) name the same frame and
 * give the same bytes.
 * bbme_temporal_filter_chain_device: chain contexts only; slots first .. first + count - 1 from ONE launch (the frame is a grid
 * dimension), frame q at d_out + q out_stride.
 * bbme_get_temporal_filtered_host: one frame as bbme_temporal_filter_device; synchronises; packed W0 x H0 bytes.
 * bbme_temporal_filter_stats: EVERY frame of the context from one launch; synchronises.  On a chain stats[4 f + k] for the slots
 * f = 0 .. pairs, otherwise stats[4 (2 p + which) + k].
 * bbme_frame_plane_device: the padded plane of frame `which` of `pair` at `level`, on any kind of context (physical in both
 * directions; on a chain slot pair + which).  Read-only: unlike bbme_level_planes_device it marks nothing as set.  A caller that
 * carries a frame across bbme_chain_advance has to copy it out on the GPU first. */
int bbme_temporal_filter_host(const uint8_t *prev, const uint8_t *cur, const uint8_t *next, int width, int height,
                              const int16_t *to_prev, const int16_t *to_next, int thr, const int *window, uint8_t *out,
                              uint8_t *weights, unsigned long long *stats4);
int bbme_cells_temporal_filter_device(bbme_ctx *ctx, const uint8_t *d_prev, const uint8_t *d_cur, const uint8_t *d_next,
                                      const int16_t *d_to_prev, const int16_t *d_to_next, int thr, const int *window, uint8_t *d_out,
                                      int out_pitch, uint8_t *d_weights, int weights_pitch, unsigned long long *d_stats4,
                                      void *hip_stream);
int bbme_temporal_filter_device(bbme_ctx *ctx, int pair, int which, int thr, uint8_t *d_out, int out_pitch, void *hip_stream);
int bbme_temporal_filter_chain_device(bbme_ctx *ctx, int first, int count, int thr, uint8_t *d_out, int out_pitch,
                                      size_t out_stride, void *hip_stream);
int bbme_get_temporal_filtered_host(bbme_ctx *ctx, int pair, int which, int thr, uint8_t *out);
int bbme_temporal_filter_stats(bbme_ctx *ctx, int thr, const int *window, unsigned long long *stats);
int bbme_frame_plane_device(bbme_ctx *ctx, int pair, int which, int level, const uint8_t **d_plane);

/* BGR TEMPORAL FILTER RULE (this project's own).  Inputs: the W x H B,G,R frame C to filter; optionally the previous frame P with
 * the cell grid GP on C that points into P; optionally the next frame N with the cell grid GN; the paddings pad_x, pad_y >= 0 with
 * W0 = W + 2 pad_x and H0 = H + 2 pad_y both even; a strength thr, 1 <= thr <= 1021.  Grids are CH x CW int16 (dx, dy) pairs,
 * CH = H0 / 2, CW = W0 / 2: the geometry a context's cells have.  Every frame is read as if zero-padded to W0 x H0: the pixel at
 * the padded position (X, Y) is frame pixel (X - pad_x, Y - pad_y), and 0 in every channel outside [0, W) x [0, H).  All
 * arithmetic is in 32-bit integers; every division is the floor division of non-negative numbers.
 * For cell (cx, cy) with origin o = (2 cx, 2 cy) and each present neighbour X (P or N) with grid G:
 *   p = o + G[cy][cx], valid when 0 <= p.x <= W0 - 2 and 0 <= p.y <= H0 - 2 (the grey rule's validity);
 *   cost_c = sum over the four pixels 0 <= i, j < 2 of |C[o + (j, i)][c] - X[p + (j, i)][c]|   for each channel c;
 *   cost = max(cost_B, cost_G, cost_R), 0..1020;
 *   w = 8 (thr - cost) / thr if the neighbour is valid and cost < thr, else 0.
 * With S = 8 + wP + wN, every channel of every pixel of the cell is
 *   out[o + (j, i)] = (8 C[o + (j, i)] + wP P[pP + (j, i)] + wN N[pN + (j, i)] + S / 2) / S.
 * The output is the UNPADDED W x H frame: with an odd padding cells straddle the frame's edge and only their pixels inside the
 * frame are written.  The weight map is the grey one, a byte wP | wN << 4 per cell of the padded view.  The statistics over a
 * window in cells: cells with wP > 0, cells with wN > 0, the sum of wP + wN, and the sum of |out - C| over the window's cells' four
 * pixels and three channels, on the padded view (a cell outside the frame is all-zero on C and counts like any other).
 * On frames with B = G = R the three costs are equal and the rule is the grey one: every channel of the frame is the unpadded
 * window of the grey result on that (zero-padded) plane, the map and the first three statistics are the grey ones, and the fourth
 * is three times the grey one.
 * WHY NOT THE LUMA'S WEIGHTS.  A 2x2 luma SAD below the strength says almost nothing about B, whose luma weight is 0.114: cells
 * that differ in B or R pass and ghost.  PSNR gain in dB of the filtered middle frame over the noisy one, interior only, worst
 * channel over the nine cases of tests/test_temporal_filter_cpu.py's quality test with one independent texture per channel and
 * the fields estimated on the luma of the noisy frames (tests/test_temporal_filter_bgr_cpu.py holds the rule's column and that the
 * luma's does worse):
 *     weights from                              two-sided    one-sided
 *     the luma SAD                                +0.71        -1.33
 *     (SAD_B + 2 SAD_G + SAD_R + 2) >> 2          +3.61        +1.76
 *     max(SAD_B, SAD_G, SAD_R)  (this rule)       +3.90        +2.14
 * The grey rule reaches 3.82 and 1.99 on the same videos in grey.  The rule reads no luma plane.
 * The context-level calls follow the grey ones in everything the rule does not change -- neighbours (image 1 its next, image 2
 * its previous one; a chain slot both where they exist), grids (the backward cells of the pair the frame is image 2 of, the forward
 * cells of the pair it is image 1 of), refusals, direction FORWARD, "changes no context state", scratch buffers of their own -- on
 * the stored colour (the COLOUR STORE above), and add: BBME_ERR_STATE when a frame they read (the frame or a neighbour the rule gives
 * it; for the statistics every frame) has no stored colour, as after a grey setter of that frame; BBME_ERR_INVALID for
 * out_pitch < 3 W, bgr_pitch < 3 W, an out_stride below one frame (out_pitch H) when count > 1.
 * bbme_temporal_filter_bgr_host: the rule on the CPU, no GPU: packed width x height frames, packed grids, out packed 3 width x
 * height, weights packed CH x CW; out, weights and stats4 each may be NULL, not all three; BBME_ERR_INVALID for an odd W0 or H0,
 * negative pads and the grey host call's refusals.
 * bbme_cells_temporal_filter_bgr_device: ANY three colour frames in HBM with one common pitch bgr_pitch >= 3 W and ANY two grids
 * of the context's cell geometry; no frames set and no estimate needed; d_out (rows out_pitch >= 3 W bytes apart, any alignment),
 * d_weights and d_stats4 each may be null, not all three; d_out must not overlap an input frame; on hip_stream (NULL = the ctx
 * stream; another stream is first ordered behind it); no host wait.  Launches with d_stats4 share one scratch buffer per context.
 * bbme_temporal_filter_bgr_device: frame `which` of `pair` from the stored colour and the context's own fields.
 * bbme_temporal_filter_bgr_chain_device: chain contexts only; slots first .. first + count - 1 from ONE launch, frame q at
 * d_out + q out_stride.
 * bbme_get_temporal_filtered_bgr_host: one frame as bbme_temporal_filter_bgr_device; synchronises; packed rows of 3 W bytes.
 * bbme_temporal_filter_bgr_stats: EVERY frame of the context from one launch; synchronises; laid out as bbme_temporal_filter_stats. */
int bbme_temporal_filter_bgr_host(const uint8_t *prev, const uint8_t *cur, const uint8_t *next, int width, int height, int pad_x,
                                  int pad_y, const int16_t *to_prev, const int16_t *to_next, int thr, const int *window,
                                  uint8_t *out, uint8_t *weights, unsigned long long *stats4);
int bbme_cells_temporal_filter_bgr_device(bbme_ctx *ctx, const uint8_t *d_prev, const uint8_t *d_cur, const uint8_t *d_next,
                                          int bgr_pitch, const int16_t *d_to_prev, const int16_t *d_to_next, int thr,
                                          const int *window, uint8_t *d_out, int out_pitch, uint8_t *d_weights, int weights_pitch,
                                          unsigned long long *d_stats4, void *hip_stream);
int bbme_temporal_filter_bgr_device(bbme_ctx *ctx, int pair, int which, int thr, uint8_t *d_out, int out_pitch, void *hip_stream);
int bbme_temporal_filter_bgr_chain_device(bbme_ctx *ctx, int first, int count, int thr, uint8_t *d_out, int out_pitch,
                                          size_t out_stride, void *hip_stream);
int bbme_get_temporal_filtered_bgr_host(bbme_ctx *ctx, int pair, int which, int thr, uint8_t *out);
int bbme_temporal_filter_bgr_stats(bbme_ctx *ctx, int thr, const int *window, unsigned long long *stats);

/* SUBPEL RULE (this project's own; the reference gets sub-pixel vectors only by estimating frames it has enlarged x4,
 * main_class.cpp:19-21, 32-33, 58-70): quarter-pel refinement of a cell grid at the planes' own resolution.  Inputs: two packed planes
 * I1 and I2 of W0 x H0 bytes (level-0 padded geometry) and a grid G of CH x CW int16 (dx, dy) integer vectors on I1 pointing into
 * I2, CH = H0 / 2, CW = W0 / 2.  All arithmetic is in 32-bit integers; >> of a negative number is the arithmetic shift.
 * Sample.  For an integer pixel position p and a quarter-pel offset q = (qx, qy): i = (qx >> 2, qy >> 2), f = (qx & 3, qy & 3),
 * P00, P10, P01, P11 the pixels of I2 at p + i + (0, 0), (1, 0), (0, 1), (1, 1), and
 *   sample(p, q) = ((4 - fx) (4 - fy) P00 + fx (4 - fy) P10 + (4 - fx) fy P01 + fx fy P11 + 8) >> 4.
 * It is exactly separable -- the horizontal sum (4 - fx) P0 + fx P1 (<= 1020) of both rows first, then the vertical one with the
 * single rounding -- and fits 16 bits throughout.
 * Cell.  For output cell (cx, cy) with origin o = (2 cx, 2 cy) and v = G[cy][cx]: the window anchor is a = o - (3, 3) (an 8 x 8
 * window around the cell) and b = a + v.  The cell is VALID when 0 <= a.x, a.x + 8 <= W0, 0 <= a.y, a.y + 8 <= H0, 2 <= b.x,
 * b.x + 10 <= W0, 2 <= b.y and b.y + 10 <= H0: every sample of every candidate then lies in the plane, with one spare pixel.
 *   cost(q) = sum over 0 <= i, j < 8 of |I1[a + (j, i)] - sample(b + (j, i), q)|,   0..16320.
 * Search.  Start with q = (0, 0) and best = cost(q).  Then for s = 2 and afterwards for s = 1: let c be the q at the start of the
 * stage; visit d in the order (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1); if cost(c + s d) < best (strictly),
 * best becomes that cost and q becomes c + s d.  That is 17 costs per valid cell and q in [-3, 3]^2.  An invalid cell keeps
 * q = (0, 0).  (Why this shape: on the Venus pair of tests/test_subpel_cpu.py a parabola through the integer SADs, a 4 x 4 or a
 * 16 x 16 window and a leading +-1-pel stage all end further from the ground truth; README.md has the table.)
 * Outputs.  The quarter-pel grid, one int16 pair per cell: sat16(4 v + q), saturation to -32768..32767 being possible on invalid
 * cells only (a valid cell has |v| < max(W0, H0)); hence BBME_ERR_UNSUPPORTED for a geometry with W0 or H0 > 8188.  The statistics
 * over a window {cx0, cy0, cw, ch} IN CELLS (NULL = all cells) are four exact 64-bit integers: valid cells, cells with
 * q != (0, 0), the sum of cost(0, 0) over the valid cells and the sum of best over the valid cells.  The statistics do not need
 * the grid to be written.
 * A context made for up-sampled frames (bbme_set_frames_*_x4) refines its 4x planes: the result is then 1/16 pel of the source.
 * A colour context refines on its luma planes.  The SUBPEL COMPENSATION RULE, the SUBPEL INTERPOLATION RULE, the BGR SUBPEL
 * INTERPOLATION RULE, the SUBPEL TEMPORAL FILTER RULE and the BGR SUBPEL TEMPORAL FILTER RULE below read quarter-pel vectors; the
 * other rules that take a cell grid
 * (integer compensation, the INTERPOLATION RULE and the BGR INTERPOLATION RULE, the TEMPORAL FILTER RULE and the BGR TEMPORAL
 * FILTER RULE) do not: they are integer.
 * Errors: BBME_ERR_INVALID for a null context or required pointer, a pair out of range, `which` not 0 or 1, q4_pitch_cells < CW, a
 * window as for the consistency rule, a d_q4 of bbme_cells_subpel_device that overlaps its input grid, an odd width or height on
 * the host call; BBME_ERR_UNSUPPORTED beyond 8188; BBME_ERR_STATE when frames are unset or a chain slot is unset, for which = 0
 * before level 0 has reached 2x2 blocks (as bbme_subsampled_flow_device) and for which = 1 without a valid pair of fields (as
 * bbme_backward_cells_device_pair).  None of these calls changes context state (grids, memo, flow, cells, backward cells, captured
 * graphs, colour store); their scratch buffers are the context's own and independent of the other getters'.  Outputs must not
 * overlap inputs.  All work on single, batched and chain contexts.
 * bbme_subpel_host: the rule on the CPU, no GPU, on packed width x height planes (both even) and a packed
 * (height / 2) x (width / 2) grid; out_q4 (packed) and stats4 each may be NULL, not both.
 * bbme_cells_subpel_device: ANY two packed planes and ANY grid in HBM of the context's level-0 / cell geometry (another
 * context's, or a caller's copies); no frames set and no estimate needed; d_q4 (rows q4_pitch_cells int16 pairs apart) and
 * d_stats4 each may be null, not both; on hip_stream (NULL = the ctx stream; another stream is first ordered behind it); no host
 * wait.  Launches with d_stats4 share one scratch buffer per context: the caller orders those it issues on different streams.
 * bbme_subpel_device: the context's own: which = 0 refines the current level-0 cells of `pair` against (image 1, image 2) -- after
 * bbme_estimate or bbme_estimate_bidirectional; in direction BACKWARD the planes exchange as for every plane-reading call --,
 * which = 1 the backward cells kept by bbme_estimate_bidirectional against (image 2, image 1).  On a chain context the planes
 * are slots pair and pair + 1.
 * bbme_get_subpel_cells_host: the same; synchronises; packed CH x CW int16 pairs.
 * bbme_subpel_stats: EVERY pair of the context from ONE launch, stats[4 p + k]; synchronises (like bbme_consistency_stats).
 * bbme_get_subpel_flow_host: the float32 (u, v) field of `pair` on the unpadded frame, packed rows: pixel (x, y) takes the
 * quarter-pel vector of cell ((pad_y + y) >> 1, (pad_x + x) >> 1) -- the cell bbme_get_subsampled_flow_host samples -- divided by 4
 * (exact in float), W x H pixels.  On a context whose frames were last set to be up-sampled (bbme_set_frames_*_x4, scale 4 of
 * bbme_set_chain_frames_*) it is the driver's subsampling in sixteenths: the (W / 4) x (H / 4) field of the source frame, pixel
 * (x, y) from cell ((pad_y + 4 y) >> 1, (pad_x + 4 x) >> 1), divided by 16.
 * Refined and expanded on the GPU; synchronises.  Ready for bbme_flo_write and bbme_calculate_mse. */
int bbme_subpel_host(const uint8_t *image1, const uint8_t *image2, int width, int height, const int16_t *cells, const int *window,
                     int16_t *out_q4, unsigned long long *stats4);
int bbme_cells_subpel_device(bbme_ctx *ctx, const uint8_t *d_image1, const uint8_t *d_image2, const int16_t *d_cells,
                             const int *window, int16_t *d_q4, int q4_pitch_cells, unsigned long long *d_stats4, void *hip_stream);
int bbme_subpel_device(bbme_ctx *ctx, int pair, int which, int16_t *d_q4, int q4_pitch_cells, void *hip_stream);
int bbme_get_subpel_cells_host(bbme_ctx *ctx, int pair, int which, int16_t *q4);
int bbme_subpel_stats(bbme_ctx *ctx, int which, const int *window, unsigned long long *stats);
int bbme_get_subpel_flow_host(bbme_ctx *ctx, int pair, int which, float *flow);

/* SUBPEL COMPENSATION RULE (this project's own; MF::draw_MVimage, motion_framework.cpp:887-905, knows integer vectors only): the
 * motion-compensated prediction along a quarter-pel grid, and its residual statistics.  Inputs: two packed planes I1 and I2 of
 * W0 x H0 bytes (I1 for the statistics only) and a quarter-pel grid Q of CH x CW int16 pairs, CH = H0 / 2, CW = W0 / 2, holding
 * vectors as the bbme_subpel_* calls write them, "4 v + q"; any int16 values are allowed.  All arithmetic is in 32-bit integers;
 * >> of a negative number is the arithmetic shift.
 * Cell.  For cell (cx, cy): o = (2 cx, 2 cy), (qx, qy) = Q[cy][cx], i = (qx >> 2, qy >> 2), f = (qx & 3, qy & 3), s = o + i.
 * The cell is COMPENSATED when 0 <= s.x, s.x + 2 + (fx != 0) <= W0, 0 <= s.y and s.y + 2 + (fy != 0) <= H0; otherwise it is
 * SKIPPED and its four pixels get `fill` (0..255).
 * Sample.  A compensated cell's pixels are MC[o + (j, k)] = sample(s + (j, k), f) for 0 <= j, k < 2: with P00, P10, P01, P11 the
 * pixels of I2 at s + (j, k) + (0, 0), (1, 0), (0, 1), (1, 1),
 *   sample = ((4 - fx) (4 - fy) P00 + fx (4 - fy) P10 + (4 - fx) fy P01 + fx fy P11 + 8) >> 4.
 * This is the SUBPEL RULE's sample, exactly separable as there (the horizontal sums first, then the vertical one with the single
 * rounding).  A tap whose weight is 0 is not part of the sample, and the validity test is exactly "every tap of non-zero weight
 * lies in the plane": no byte outside the W0 x H0 plane is read.
 * Statistics: the four of the compensation rule, over a window {x0, y0, w, h} in PIXELS of the plane (NULL = the whole plane) --
 * the window of bbme_compensation_error, not the cell window of bbme_subpel_stats.  sse = sum (MC - I1)^2 and sad = sum |MC - I1|
 * over the window pixels of compensated cells, pixels = their count, skipped = the count of window pixels of skipped cells.  All
 * four are exact 64-bit integers and do not depend on `fill`.  A window may cut cells: each pixel counts on its own.
 * Property.  With Q = 4 G for an integer grid G, the frame and the statistics are those of the compensation rule at level 0 with
 * block 2 and grid_block 2, bit for bit.
 * A context made for up-sampled frames compensates its 4x planes, a colour context its luma planes (its colour frames: the BGR
 * COMPENSATION RULE below).
 * Errors: BBME_ERR_INVALID for a null context or required pointer, a pair out of range, `which` not 0 or 1, a fill outside
 * 0..255, a window not inside the plane, q4_pitch_cells < CW, out_pitch < W0, a d_out of bbme_cells_subpel_compensate_device
 * that overlaps an input plane, an odd width or height on the host call; for the context's own calls BBME_ERR_UNSUPPORTED beyond
 * 8188 and BBME_ERR_STATE exactly as bbme_subpel_device.  None of the device calls changes context state (grids, memo, flow,
 * cells, backward cells, captured graphs, colour store); their scratch buffers are the context's own and independent of the
 * other getters'.  Outputs must not overlap inputs.  All work on single, batched and chain contexts.
 * bbme_subpel_compensate_host: the rule on the CPU, no GPU, on packed width x height planes (both even) and a packed
 * (height / 2) x (width / 2) grid; image1 may be NULL without statistics; out (packed) and stats4 each may be NULL, not both.
 * bbme_cells_subpel_compensate_device: ANY packed planes and ANY quarter-pel grid in HBM of the context's level-0 geometry, grid
 * rows q4_pitch_cells int16 pairs apart (bbme_subpel_device's strided output can be fed straight in); no frames set and no
 * estimate needed; d_image1 may be null without d_stats4; d_out (rows out_pitch bytes apart) and d_stats4 each may be null, not
 * both; on hip_stream (NULL = the ctx stream; another stream is first ordered behind it); no host wait.  It has no size limit of
 * its own (s is computed in 32 bits from any int16).  Launches with d_stats4 share one scratch buffer per context: the caller
 * orders those it issues on different streams.
 * bbme_subpel_compensate_device: the context's own: the cells of `pair` are refined (bbme_subpel_device's `which`) into a
 * quarter-pel buffer of the context's, allocated at first use, then compensated from it: which = 0 predicts image 1 from image 2
 * along the current cells (in direction BACKWARD the planes exchange as for every plane-reading call), which = 1 predicts image 2
 * from image 1 along the backward cells of bbme_estimate_bidirectional.  On a chain context the planes are slots pair and
 * pair + 1.  The caller orders calls for the same pair that it issues on different streams.
 * bbme_get_subpel_compensated_host: the same; synchronises; the packed padded W0 x H0 plane.
 * bbme_subpel_compensation_error: EVERY pair of the context, stats[4 p + k], from one refinement launch and one compensation
 * launch over all pairs; synchronises.  The statistics are against image 1 for which = 0 and against image 2 for which = 1. */
int bbme_subpel_compensate_host(const uint8_t *image1, const uint8_t *image2, int width, int height, const int16_t *q4, int fill,
                                const int *window, uint8_t *out, unsigned long long *stats4);
int bbme_cells_subpel_compensate_device(bbme_ctx *ctx, const uint8_t *d_image1, const uint8_t *d_image2, const int16_t *d_q4,
                                        int q4_pitch_cells, int fill, const int *window, uint8_t *d_out, int out_pitch,
                                        unsigned long long *d_stats4, void *hip_stream);
int bbme_subpel_compensate_device(bbme_ctx *ctx, int pair, int which, int fill, uint8_t *d_out, int out_pitch, void *hip_stream);
int bbme_get_subpel_compensated_host(bbme_ctx *ctx, int pair, int which, int fill, uint8_t *out);
int bbme_subpel_compensation_error(bbme_ctx *ctx, int which, const int *window, unsigned long long *stats);

/* SUBPEL INTERPOLATION RULE (this project's own): the frame at phase num / den between frame 1 (phase 0) and frame 2 (phase 1) of
 * a pair, motion-compensated from both fields at QUARTER-PEL positions.  It is the INTERPOLATION RULE with every position in
 * quarter pels and every cell sampled as in the SUBPEL COMPENSATION RULE: the integer rule places a cell at origin - round(num v /
 * den) in whole pixels, so a block that moves 1 px per frame cannot be put at phase 1 / 2; this one can.
 * Inputs: the level-0 padded planes I1 and I2 (W0 x H0 bytes), a quarter-pel grid QF on frame 1 (forward) and, optionally, a
 * quarter-pel grid QB on frame 2 (backward), CH x CW int16 pairs each (CH = H0 / 2, CW = W0 / 2) holding vectors as the
 * bbme_subpel_* calls write them, "4 v + q"; any int16 values are allowed; and the phase, 2 <= den <= 256 and 0 < num < den.  All
 * arithmetic is in 32-bit integers; >> of a negative number is the arithmetic shift; den / 2 is the integer half; floor_div rounds
 * towards minus infinity.
 * Output cell (cx, cy) with origin o = (2 cx, 2 cy) has up to three hypotheses, in this order, all in QUARTER pels:
 *   k = 0: v = QF[cy][cx];   k = 1: v = -QB[cy][cx] (absent without QB);   k = 2: v = (0, 0).
 * For a hypothesis v = (vx, vy): the shift s = (floor_div(num vx + den / 2, den), floor_div(num vy + den / 2, den)),
 * P1 = 4 o - s and P2 = P1 + v (so P2 - P1 = v exactly).
 * Samples.  For a quarter-pel position P: i = (P.x >> 2, P.y >> 2), f = (P.x & 3, P.y & 3), and the cell's four pixels are
 * S[j, r] = sample(i + (j, r), f) for 0 <= j, r < 2: with P00, P10, P01, P11 the plane's pixels at i + (j, r) + (0, 0), (1, 0),
 * (0, 1), (1, 1),
 *   sample = ((4 - fx) (4 - fy) P00 + fx (4 - fy) P10 + (4 - fx) fy P01 + fx fy P11 + 8) >> 4.
 * This is the SUBPEL RULE's sample, exactly separable as there (the horizontal sums first, then the vertical one with the single
 * rounding).  S1 samples I1 at P1, S2 samples I2 at P2.  A tap whose weight is 0 is not part of the sample.
 * Validity.  A hypothesis is valid when every tap of non-zero weight of both cells lies in the plane: for each of P1 and P2,
 * 0 <= i.x, i.x + 2 + (fx != 0) <= W0, 0 <= i.y and i.y + 2 + (fy != 0) <= H0 (k = 2 always is).  No byte outside the W0 x H0
 * planes is read.
 * Its cost is the sum over the four pixels of |S1 - S2| on the ROUNDED samples, 0..1020.  The valid hypothesis of the smallest
 * cost is selected; of equal costs the earliest.  With its S1 and S2, out[oy + r][ox + j] = ((den - num) S1[j, r] + num S2[j, r]
 * + den / 2) / den for 0 <= j, r < 2.
 * The selection map holds one byte k per cell.  The statistics over a window {cx0, cy0, cw, ch} IN CELLS (NULL = all cells) are
 * four exact 64-bit integers: cells that selected k = 0, k = 1, k = 2, and the sum of the selected costs.
 * One call makes `count` consecutive phases num0 .. num0 + count - 1 of one den in ONE launch (the phase is a grid dimension;
 * planes and grids come from L2 for all but the first): frame q at d_out + q out_stride, its map at d_sel + q sel_stride, its
 * statistics at d_stats4[4 q ..].
 * Properties.  (1) Integer cases reproduce the INTERPOLATION RULE: with QF = 4 F and QB = 4 B for integer grids F and B, if den
 * divides num v componentwise for every hypothesis v of every cell, the frame, the map and the statistics are those of the
 * INTERPOLATION RULE on F and B, bit for bit (every fraction is 0 then).  (2) With both grids zero the result is the in-place
 * blend of the INTERPOLATION RULE on zero grids.  (3) The grid call has no size limit of its own: |num v| <= (den - 1) 32768 for
 * every int16 v, -(-32768) included, so num v + den / 2 + 32768 den stays below 2^24, where the multiply-shift by
 * floor(2^32 / den) + 1 is the exact quotient, and P1 and P2 are computed in 32 bits from any int16.
 * A context made for up-sampled frames (bbme_set_frames_*_x4) interpolates its 4x planes, a colour context its luma planes (the
 * BGR SUBPEL INTERPOLATION RULE below makes the colour frame).
 * Errors: those of the INTERPOLATION RULE's calls, and q4_pitch_cells < CW; for the three calls on the context's own fields
 * BBME_ERR_STATE exactly as bbme_interpolate_device and BBME_ERR_UNSUPPORTED beyond 8188 as bbme_subpel_device.  None of these
 * calls changes context state; their scratch buffers are the context's own and independent of the other getters'.  All work on
 * single, batched and chain contexts; in direction BACKWARD the two planes exchange, as for every plane-reading call.
 * bbme_subpel_interpolate_host: the rule on the CPU, no GPU, on packed width x height planes (both even) and packed
 * (height / 2) x (width / 2) grids (qb may be NULL); out, sel (packed) and stats4 each may be NULL, not all three.
 * bbme_cells_subpel_interpolate_device: the context's planes of `pair` and ANY two quarter-pel grids in HBM of its cell geometry,
 * rows of both q4_pitch_cells int16 pairs apart (bbme_subpel_device's strided output can be fed straight in; d_qb may be null);
 * d_out, d_sel and d_stats4 each may be null, not all three; on hip_stream (NULL = the ctx stream; another stream is first ordered
 * behind it); no host wait; needs no valid pair of fields.  Launches with d_stats4 share one scratch buffer per context: the
 * caller orders those it issues on different streams.
 * bbme_subpel_interpolate_device: the context's own, frames only: the forward cells (bbme_subpel_device's which = 0) and the kept
 * backward cells (which = 1) of `pair` are refined into a quarter-pel buffer of the context's (two packed grids per pair, allocated
 * at first use, not the compensation's), then interpolated from it.  The caller orders calls for the same pair that it issues on
 * different streams.
 * bbme_get_subpel_interpolated_host: one phase of the same; synchronises; packed W0 x H0 bytes.
 * bbme_subpel_interpolation_stats: EVERY pair, stats[4 p + k], from two refinement launches and one interpolation launch over all
 * pairs; synchronises. */
int bbme_subpel_interpolate_host(const uint8_t *image1, const uint8_t *image2, int width, int height, const int16_t *qf,
                                 const int16_t *qb, int num, int den, const int *window, uint8_t *out, uint8_t *sel,
                                 unsigned long long *stats4);
int bbme_cells_subpel_interpolate_device(bbme_ctx *ctx, int pair, const int16_t *d_qf, const int16_t *d_qb, int q4_pitch_cells,
                                         int num0, int count, int den, const int *window, uint8_t *d_out, int out_pitch,
                                         size_t out_stride, uint8_t *d_sel, int sel_pitch, size_t sel_stride,
                                         unsigned long long *d_stats4, void *hip_stream);
int bbme_subpel_interpolate_device(bbme_ctx *ctx, int pair, int num0, int count, int den, uint8_t *d_out, int out_pitch,
                                   size_t out_stride, void *hip_stream);
int bbme_get_subpel_interpolated_host(bbme_ctx *ctx, int pair, int num, int den, uint8_t *out);
int bbme_subpel_interpolation_stats(bbme_ctx *ctx, int num, int den, const int *window, unsigned long long *stats);

/* BGR SUBPEL INTERPOLATION RULE (this project's own): the colour frame at phase num / den at QUARTER-PEL positions; the SUBPEL
 * INTERPOLATION RULE's selection with the BGR INTERPOLATION RULE's output.
 * Inputs: those of the SUBPEL INTERPOLATION RULE -- the level-0 padded LUMA planes I1, I2 (W0 x H0), the quarter-pel grids QF and,
 * optionally, QB, the phase num / den -- and those the BGR INTERPOLATION RULE adds: the two colour frames C1, C2 (W x H pixels of
 * B,G,R) whose lumas the planes hold at (pad_x, pad_y): W0 = W + 2 pad_x, H0 = H + 2 pad_y.
 * Selection is EXACTLY the SUBPEL INTERPOLATION RULE's, on the luma planes, in padded quarter-pel coordinates: hypotheses, their
 * order, the shift s, P1, P2, validity, the cost on the rounded luma samples and ties are unchanged, so the selection map and the
 * statistics of a colour frame are those bbme_cells_subpel_interpolate_device returns; the colour calls make neither.
 * The output is the UNPADDED W x H B,G,R frame.  Output pixel (x, y) has the padded position (X, Y) = (x + pad_x, y + pad_y) and
 * belongs to cell (X >> 1, Y >> 1) at offset (j, r) = (X & 1, Y & 1).  With that cell's selected P1 and P2, for P in {P1, P2}:
 *     t = (P.x >> 2, P.y >> 2) + (j, r) - (pad_x, pad_y)   (frame coordinates),   f = (P.x & 3, P.y & 3),
 * and for every channel, with T00, T10, T01, T11 the frame's pixels at t + (0, 0), (1, 0), (0, 1), (1, 1),
 *     sample = ((4 - fx) (4 - fy) T00 + fx (4 - fy) T10 + (4 - fx) fy T01 + fx fy T11 + 8) >> 4.
 * A tap outside [0, W) x [0, H) reads 0 in every channel: the zero border the luma planes have (a selected hypothesis is valid, so
 * such a tap lies in that border).  A tap of weight 0 is not read; no byte outside the colour frames is ever read.  With S1 the
 * sample of C1 at P1 and S2 the one of C2 at P2,
 *     out[y][x][c] = ((den - num) S1 + num S2 + den / 2) / den.
 * pad_x and pad_y may be odd: cells then straddle the frame's edge and only their pixels inside the frame are written.
 * Properties.  (1) On frames with B = G = R every channel of the result is the unpadded window of the grey SUBPEL INTERPOLATION
 * RULE's result, bit for bit.  (2) With QF = 4 F and QB = 4 B for integer grids F and B, if den divides num v componentwise for
 * every hypothesis v of every cell, the result is the BGR INTERPOLATION RULE's on F and B, bit for bit.  (3) With both grids zero
 * the result is the in-place blend of the two colour frames.
 * `count` consecutive phases come from one launch, frame q at d_out + q out_stride, rows out_pitch bytes apart (any alignment).
 * Errors: the union of bbme_cells_interpolate_bgr_device's and bbme_cells_subpel_interpolate_device's: BBME_ERR_INVALID for a null
 * context or required pointer, pair, den, num0, count, q4_pitch_cells < CW, bgr_pitch < 3 W, out_pitch < 3 W, a stride below one
 * frame when count > 1, exactly one of d_bgr1 / d_bgr2 null; BBME_ERR_STATE when frames are unset, when stored colour is asked for
 * and either frame of the pair has none, and for the two context-level calls without a valid pair of fields;
 * BBME_ERR_UNSUPPORTED beyond 8188 for the two context-level calls (as bbme_subpel_device).  None of these calls changes context
 * state.  All work on single, batched and chain contexts; in direction BACKWARD the two colour frames exchange together with the
 * two planes (callers' frames too).
 * bbme_subpel_interpolate_bgr_host: the rule on the CPU, no GPU: packed padded_w x padded_h luma planes (both even), packed
 * width x height colour frames, packed (padded_h / 2) x (padded_w / 2) quarter-pel grids (qb may be NULL), out packed 3 width x
 * height; BBME_ERR_INVALID unless padded_w = width + 2 pad_x and padded_h = height + 2 pad_y with pads >= 0.
 * bbme_cells_subpel_interpolate_bgr_device: the context's planes of `pair`, ANY two quarter-pel grids in HBM of its cell geometry,
 * rows of both q4_pitch_cells int16 pairs apart (d_qb may be null), and either the stored colour (d_bgr1 = d_bgr2 = null) or a
 * caller's two frames in HBM, rows bgr_pitch bytes apart; on hip_stream (NULL = the ctx stream; another stream is first ordered
 * behind it); no host wait; needs no valid pair of fields.
 * bbme_subpel_interpolate_bgr_device: the context's own: both fields of `pair` refined into the context's quarter-pel buffer
 * exactly as bbme_subpel_interpolate_device does, then one launch on the stored colour.  The caller orders calls for the same pair
 * that it issues on different streams.
 * bbme_get_subpel_interpolated_bgr_host: one phase of the same; synchronises; packed rows of 3 W bytes. */
int bbme_subpel_interpolate_bgr_host(const uint8_t *luma1, const uint8_t *luma2, int padded_w, int padded_h, const uint8_t *bgr1,
                                     const uint8_t *bgr2, int width, int height, int pad_x, int pad_y, const int16_t *qf,
                                     const int16_t *qb, int num, int den, uint8_t *out);
int bbme_cells_subpel_interpolate_bgr_device(bbme_ctx *ctx, int pair, const int16_t *d_qf, const int16_t *d_qb, int q4_pitch_cells,
                                             const uint8_t *d_bgr1, const uint8_t *d_bgr2, int bgr_pitch, int num0, int count,
                                             int den, uint8_t *d_out, int out_pitch, size_t out_stride, void *hip_stream);
int bbme_subpel_interpolate_bgr_device(bbme_ctx *ctx, int pair, int num0, int count, int den, uint8_t *d_out, int out_pitch,
                                       size_t out_stride, void *hip_stream);
int bbme_get_subpel_interpolated_bgr_host(bbme_ctx *ctx, int pair, int num, int den, uint8_t *out);

/* SUBPEL TEMPORAL FILTER RULE (this project's own): the TEMPORAL FILTER RULE with each neighbour's cell taken at a QUARTER-PEL
 * position, as in the SUBPEL COMPENSATION RULE.  Inputs: those of the TEMPORAL FILTER RULE -- the plane C, optionally P and / or N
 * (packed W0 x H0 bytes), a strength thr, 1 <= thr <= 1021 -- except that the two grids QP (on C, into P) and QN (on C, into N) hold
 * quarter-pel vectors, CH x CW int16 (qx, qy) pairs as bbme_subpel_* writes them; any int16 is allowed.  All arithmetic is in 32-bit
 * integers, `>>` of a negative number is the arithmetic shift, every division the floor division of non-negative numbers.
 * For output cell (cx, cy) with origin o = (2 cx, 2 cy) and each present neighbour X with grid Q:
 *   (qx, qy) = Q[cy][cx], i = (qx >> 2, qy >> 2), f = (qx & 3, qy & 3), s = o + i;
 *   the neighbour is valid when 0 <= s.x, s.x + 2 + (fx != 0) <= W0, 0 <= s.y and s.y + 2 + (fy != 0) <= H0: every tap of non-zero
 *   weight lies in the plane.  A tap of weight 0 is not read; no byte outside W0 x H0 is read;
 *   X'[j, k] = sample(s + (j, k), f) for 0 <= j, k < 2, the SUBPEL RULE's sample with its single rounding, (... + 8) >> 4;
 *   cost = sum over the four ROUNDED samples of |C[o + (j, k)] - X'[j, k]|, 0..1020;
 *   w = 8 (thr - cost) / thr if the neighbour is valid and cost < thr, else 0.
 * With S = 8 + wP + wN (8..24),
 *   out[o + (j, k)] = (8 C[o + (j, k)] + wP P'[j, k] + wN N'[j, k] + S / 2) / S.
 * The weight map (wP | wN << 4, one byte per cell) and the four statistics over a window in cells (cells with wP > 0, cells with
 * wN > 0, the sum of wP + wN, the sum of |out - C|) are the TEMPORAL FILTER RULE's.
 * Properties.  (1) With QP = 4 GP and QN = 4 GN for integer grids the frame, the map and the statistics are the TEMPORAL FILTER
 * RULE's on GP and GN, bit for bit (the validity test reduces to 0 <= p <= W0 - 2 / H0 - 2).  (2) With equal planes and zero grids
 * the frame is unchanged and every present weight is 8.  (3) The grid call has no size limit of its own: s is computed in 32 bits
 * from any int16.
 * On a context with its own fields the grid into the previous frame is the BACKWARD cells of the pair the frame is image 2 of and
 * the grid into the next frame the FORWARD cells of the pair it is image 1 of, each refined by the SUBPEL RULE (K10) into
 * quarter-pel buffers of the context's own, allocated at first use.  A context made for up-sampled frames filters its 4x planes; a
 * colour context its luma planes.  The BGR TEMPORAL FILTER RULE stays integer.
 * Errors: those of the TEMPORAL FILTER RULE's calls, plus BBME_ERR_INVALID for q4_pitch_cells < CW and BBME_ERR_UNSUPPORTED beyond
 * W0 or H0 8188 for the four context-level calls (as bbme_subpel_device); BBME_ERR_STATE for those without a valid pair of
 * fields; BBME_ERR_UNSUPPORTED for bbme_subpel_temporal_filter_chain_device off a chain.  None of these calls changes context
 * state (grids, memo, flow, cells, backward cells, captured graphs, colour store); the statistics scratch and the quarter-pel
 * buffers are their own.  The caller orders context-level calls that it issues on different streams.
 * bbme_subpel_temporal_filter_host: the rule on the CPU, no GPU, on packed width x height planes (both even) and packed
 * (height / 2) x (width / 2) quarter-pel grids; out, weights (packed) and stats4 each may be NULL, not all three.
 * bbme_cells_subpel_temporal_filter_device: ANY three packed planes and ANY two quarter-pel grids in HBM of the context's level-0 /
 * cell geometry, rows of both grids q4_pitch_cells int16 pairs apart (bbme_subpel_device's output goes straight in); otherwise as
 * bbme_cells_temporal_filter_device; no host wait.
 * bbme_subpel_temporal_filter_device: frame `which` of `pair` with the neighbours bbme_temporal_filter_device gives it: the
 * integer grids it needs refined (one K10 launch each), then one filter launch.
 * bbme_subpel_temporal_filter_chain_device: chain contexts only; at most two refinement launches (the forward cells of all pairs
 * the run needs, the backward cells of all pairs it needs), then ONE filter launch for slots first .. first + count - 1, frame q
 * at d_out + q out_stride.
 * bbme_get_subpel_temporal_filtered_host: one frame as bbme_subpel_temporal_filter_device; synchronises; packed W0 x H0 bytes.
 * bbme_subpel_temporal_filter_stats: EVERY frame of the context from one filter launch; synchronises; laid out as
 * bbme_temporal_filter_stats. */
int bbme_subpel_temporal_filter_host(const uint8_t *prev, const uint8_t *cur, const uint8_t *next, int width, int height,
                                     const int16_t *q_to_prev, const int16_t *q_to_next, int thr, const int *window, uint8_t *out,
                                     uint8_t *weights, unsigned long long *stats4);
int bbme_cells_subpel_temporal_filter_device(bbme_ctx *ctx, const uint8_t *d_prev, const uint8_t *d_cur, const uint8_t *d_next,
                                             const int16_t *d_q_to_prev, const int16_t *d_q_to_next, int q4_pitch_cells, int thr,
                                             const int *window, uint8_t *d_out, int out_pitch, uint8_t *d_weights, int weights_pitch,
                                             unsigned long long *d_stats4, void *hip_stream);
int bbme_subpel_temporal_filter_device(bbme_ctx *ctx, int pair, int which, int thr, uint8_t *d_out, int out_pitch, void *hip_stream);
int bbme_subpel_temporal_filter_chain_device(bbme_ctx *ctx, int first, int count, int thr, uint8_t *d_out, int out_pitch,
                                             size_t out_stride, void *hip_stream);
int bbme_get_subpel_temporal_filtered_host(bbme_ctx *ctx, int pair, int which, int thr, uint8_t *out);
int bbme_subpel_temporal_filter_stats(bbme_ctx *ctx, int thr, const int *window, unsigned long long *stats);

/* BGR SUBPEL TEMPORAL FILTER RULE (this project's own): the BGR TEMPORAL FILTER RULE with each neighbour's cell taken at a
 * QUARTER-PEL position, the position taken exactly as the SUBPEL TEMPORAL FILTER RULE takes it, but on the zero-padded view of the
 * colour frames.  Inputs: those of the BGR TEMPORAL FILTER RULE -- the W x H B,G,R frame C, optionally P and / or N, the paddings
 * pad_x, pad_y >= 0 with W0 = W + 2 pad_x and H0 = H + 2 pad_y both even, a strength thr, 1 <= thr <= 1021 -- except that the two
 * grids QP (on C, into P) and QN (on C, into N) hold quarter-pel vectors, CH x CW int16 (qx, qy) pairs as bbme_subpel_* writes
 * them; any int16 is allowed.  All arithmetic is in 32-bit integers, `>>` of a negative number is the arithmetic shift, every
 * division the floor division of non-negative numbers.
 * For cell (cx, cy) with origin o = (2 cx, 2 cy) in the padded view and each present neighbour X with grid Q:
 *   (qx, qy) = Q[cy][cx], i = (qx >> 2, qy >> 2), f = (qx & 3, qy & 3), s = o + i;
 *   the neighbour is valid when 0 <= s.x, s.x + 2 + (fx != 0) <= W0, 0 <= s.y and s.y + 2 + (fy != 0) <= H0: the grey subpel
 *   filter's validity, on the padded view;
 *   X'[j, k][c] = ((4 - fx)(4 - fy) T00 + fx (4 - fy) T10 + (4 - fx) fy T01 + fx fy T11 + 8) >> 4 for 0 <= j, k < 2 and every channel
 *   c, T.. the taps at the padded positions s + (j, k) + {(0, 0), (1, 0), (0, 1), (1, 1)}.  A tap at the padded position (X, Y) is
 *   frame pixel (X - pad_x, Y - pad_y), and 0 in every channel outside [0, W) x [0, H).  A tap of weight 0 is not read; no byte
 *   outside the frames is ever read;
 *   cost_c = sum over the four ROUNDED samples of |C[o + (j, k)][c] - X'[j, k][c]|;
 *   cost = max(cost_B, cost_G, cost_R), 0..1020;
 *   w = 8 (thr - cost) / thr if the neighbour is valid and cost < thr, else 0.
 * With S = 8 + wP + wN (8..24), every channel of every pixel of the cell is
 *   out[o + (j, k)] = (8 C[o + (j, k)] + wP P'[j, k] + wN N'[j, k] + S / 2) / S.
 * The output is the UNPADDED W x H frame: with an odd padding cells straddle the frame's edge and only their pixels inside the
 * frame are written.  The weight map (wP | wN << 4, one byte per cell of the padded view) and the four statistics over a window in
 * cells are the BGR TEMPORAL FILTER RULE's: the fourth is the sum of |out - C| over three channels, on the padded view.
 * Properties.  (1) On frames with B = G = R every channel is the unpadded window of the SUBPEL TEMPORAL FILTER RULE's result on the
 * zero-padded plane; the map and the first three statistics are equal and the fourth is three times the grey one.  (2) With
 * QP = 4 GP and QN = 4 GN for integer grids the frame, the map and the statistics are the BGR TEMPORAL FILTER RULE's on GP and GN,
 * bit for bit.  (3) With equal frames and zero grids the frame is unchanged and every present weight is 8.  (4) The grid call has
 * no size limit of its own: s is computed in 32 bits from any int16.
 * WHAT IT BUYS.  PSNR gain in dB of the filtered middle frame over the noisy one, worst channel, interior only, one independent
 * texture per channel, over two sizes and three noise levels (tests/test_subpel_temporal_filter_bgr_cpu.py holds these):
 *     motion per frame (quarter pels)     BGR rule, two- / one-sided        this rule, two- / one-sided
 *     whole pixels                        +4.3..+4.7 / +2.7..+2.8           the same frames
 *     half pixels                         +2.1..+4.5 / +0.3..+2.4           +5.2..+6.7 / +3.6..+4.2
 *     odd quarter pels                    +4.0..+4.6 / +1.4..+2.7           +5.3..+6.2 / +3.5..+3.9
 * On a context with its own fields the grids are those the SUBPEL TEMPORAL FILTER RULE's context calls use: the backward cells of
 * the pair the frame is image 2 of and the forward cells of the pair it is image 1 of, each refined by the SUBPEL RULE (K10) on the
 * LUMA planes into the context's quarter-pel buffers; the filter then reads only the stored colour (the COLOUR STORE above).
 * Errors: the union of both families'.  BBME_ERR_INVALID for bgr_pitch or out_pitch < 3 W, an out_stride below one frame when
 * count > 1, q4_pitch_cells < CW, thr outside 1..1021, a bad window, an output that overlaps an input frame; BBME_ERR_STATE without
 * a valid pair of fields or when a frame the call reads has no stored colour; BBME_ERR_UNSUPPORTED beyond W0 or H0 8188 for the
 * four context-level calls and for bbme_subpel_temporal_filter_bgr_chain_device off a chain.  None of these calls changes context
 * state (grids, memo, flow, cells, backward cells, captured graphs, colour store); the statistics scratch is their own, the
 * quarter-pel buffers are those of the grey calls (the same cells of the same planes: the same vectors).
 * bbme_subpel_temporal_filter_bgr_host: the rule on the CPU, no GPU: bbme_temporal_filter_bgr_host's arguments, the grids
 * quarter-pel.
 * bbme_cells_subpel_temporal_filter_bgr_device: ANY three colour frames in HBM with one common pitch bgr_pitch >= 3 W and ANY two
 * quarter-pel grids of the context's cell geometry, rows of both grids q4_pitch_cells int16 pairs apart; otherwise as
 * bbme_cells_temporal_filter_bgr_device; no host wait.
 * bbme_subpel_temporal_filter_bgr_device: frame `which` of `pair`: the integer grids it needs refined (one K10 launch each), then
 * one filter launch.
 * bbme_subpel_temporal_filter_bgr_chain_device: chain contexts only; at most two refinement launches, then ONE filter launch for
 * slots first .. first + count - 1, frame q at d_out + q out_stride.
 * bbme_get_subpel_temporal_filtered_bgr_host: one frame as bbme_subpel_temporal_filter_bgr_device; synchronises; packed rows of
 * 3 W bytes.
 * bbme_subpel_temporal_filter_bgr_stats: EVERY frame of the context from one filter launch; synchronises; laid out as
 * bbme_temporal_filter_stats. */
int bbme_subpel_temporal_filter_bgr_host(const uint8_t *prev, const uint8_t *cur, const uint8_t *next, int width, int height, int pad_x,
                                         int pad_y, const int16_t *q_to_prev, const int16_t *q_to_next, int thr, const int *window,
                                         uint8_t *out, uint8_t *weights, unsigned long long *stats4);
int bbme_cells_subpel_temporal_filter_bgr_device(bbme_ctx *ctx, const uint8_t *d_prev, const uint8_t *d_cur, const uint8_t *d_next,
                                                 int bgr_pitch, const int16_t *d_q_to_prev, const int16_t *d_q_to_next,
                                                 int q4_pitch_cells, int thr, const int *window, uint8_t *d_out, int out_pitch,
                                                 uint8_t *d_weights, int weights_pitch, unsigned long long *d_stats4, void *hip_stream);
int bbme_subpel_temporal_filter_bgr_device(bbme_ctx *ctx, int pair, int which, int thr, uint8_t *d_out, int out_pitch,
                                           void *hip_stream);
int bbme_subpel_temporal_filter_bgr_chain_device(bbme_ctx *ctx, int first, int count, int thr, uint8_t *d_out, int out_pitch,
                                                 size_t out_stride, void *hip_stream);
int bbme_get_subpel_temporal_filtered_bgr_host(bbme_ctx *ctx, int pair, int which, int thr, uint8_t *out);
int bbme_subpel_temporal_filter_bgr_stats(bbme_ctx *ctx, int thr, const int *window, unsigned long long *stats);

/* CELL COMPOSITION RULE (this project's own): the field from frame X into frame Z, two frames on, from the field of X into Y and
 * the field of Y into Z.  Inputs: grid A on X into Y and grid B on Y into Z, both CH x CW int16 (x, y) pairs, rows a_pitch_cells
 * and b_pitch_cells pairs apart; a unit shift u, 0 (the vectors are pixels) or 2 (quarter pels).  Any int16 is allowed.  All
 * arithmetic is in 32-bit integers, `>>` of a negative number is the arithmetic shift.
 * For cell (cx, cy) with a = A[cy][cx]:
 *   t  = ((2 cx, 2 cy) << u) + a                                   where the cell's origin lands in Y, in the vectors' unit;
 *   c' = ((t.x + (1 << u)) >> (u + 1), (t.y + (1 << u)) >> (u + 1)) the cell of Y whose origin is nearest, ties upward;
 *   c' is clamped to 0 .. CW - 1 and 0 .. CH - 1: no index leaves the grid;
 *   out[cy][cx] = sat16(a + B[c']), each component saturated to -32768 .. 32767.
 * Two statistics over a window in cells: cells whose c' was clamped (in either coordinate), cells that saturated (in either
 * component).
 * Properties.  (1) B = 0 gives A; A = 0 gives B.  (2) With u = 2, A = 4 GA and B = 4 GB the result is 4 x the result of u = 0 on GA
 * and GB wherever neither saturates (c' is the same cell).  (3) Any int16 is legal.
 * The composed grid is an INTEGER guess of a distance-2 field: the WIDE TEMPORAL FILTER RULE's context calls refine it by the
 * SUBPEL RULE against the real frame pair before they use it.
 * Errors: BBME_ERR_INVALID for a null context or required pointer, a pitch < CW, u not 0 or 2, a window as for the consistency
 * rule, an output that overlaps an input, slots or a side without a composition; BBME_ERR_UNSUPPORTED for
 * bbme_compose_chain_device off a chain; BBME_ERR_STATE for it without frames and a valid bidirectional estimate.  None of these
 * calls changes context state; the statistics scratch is their own.
 * bbme_compose_host: the rule on the CPU, no GPU; out (rows out_pitch_cells pairs apart) and stats2 each may be NULL, not both.
 * bbme_cells_compose_device: ANY two grids in HBM of the context's cell geometry, on hip_stream (NULL = the context's), ordered
 * behind the context's stream; no host wait.  d_out must not overlap d_a or d_b.
 * bbme_compose_chain_device: chain contexts only, after bbme_estimate_bidirectional; ONE launch, the frame a grid dimension, for
 * slots first .. first + count - 1, slot first + q at d_out + q out_stride_cells pairs.  side = +1: for slot f the grid into slot
 * f + 2, compose(forward cells of pair f, forward cells of pair f + 1), u = 0; every slot must be <= the last slot - 2.
 * side = -1: the grid into slot f - 2, compose(backward cells of pair f - 1, backward cells of pair f - 2); every slot >= 2. */
int bbme_compose_host(const int16_t *a, int a_pitch_cells, const int16_t *b, int b_pitch_cells, int cells_w, int cells_h,
                      int unit_shift, const int *window, int16_t *out, int out_pitch_cells, unsigned long long *stats2);
int bbme_cells_compose_device(bbme_ctx *ctx, const int16_t *d_a, int a_pitch_cells, const int16_t *d_b, int b_pitch_cells,
                              int unit_shift, const int *window, int16_t *d_out, int out_pitch_cells, unsigned long long *d_stats2,
                              void *hip_stream);
int bbme_compose_chain_device(bbme_ctx *ctx, int first, int count, int side, int16_t *d_out, int out_pitch_cells,
                              size_t out_stride_cells, void *hip_stream);

/* WIDE TEMPORAL FILTER RULE (this project's own): the SUBPEL TEMPORAL FILTER RULE with up to FOUR neighbours, two frames on each
 * side.  Neighbour k = 0 .. 3 is P1 (the previous frame), N1 (the next), P2 (two back), N2 (two on): a packed W0 x H0 plane X_k
 * and a quarter-pel grid Q_k on C into X_k (CH x CW int16 pairs, rows q4_pitch_cells pairs apart, one pitch for all; any int16).
 * A neighbour is present when both its plane and its grid are given; at least one must be present.  Grey planes only.
 * Each neighbour's validity, rounded samples X'_k, cost and weight w_k (0..8) are exactly the SUBPEL TEMPORAL FILTER RULE's, each
 * independent of the other neighbours.  With S = 8 + sum of w_k (8..40),
 *   out[o + (j, k)] = (8 C[o + (j, k)] + sum over k of w_k X'_k[j, k] + S / 2) / S         the numerator is at most 10220.
 * The weight map is one uint16 per cell, w_0 | w_1 << 4 | w_2 << 8 | w_3 << 12.  Six statistics over a window in cells: cells
 * with w_k > 0 for k = 0 .. 3, the sum of all weights, the sum of |out - C|.
 * Properties.  (1) With neighbours 2 and 3 absent the frame, the low byte of the map and statistics 0, 1, 4, 5 are the SUBPEL
 * TEMPORAL FILTER RULE's, bit for bit; with 4 x integer grids therefore the TEMPORAL FILTER RULE's.  (2) Equal planes and zero
 * grids leave the frame unchanged, every present weight 8.  (3) Exchanging two neighbours' (plane, grid) exchanges their nibbles
 * and their counters and nothing else.
 * On a CHAIN context with its own fields slot f uses, as far as the chain has them, slots f - 1 and f + 1 with the grids the
 * SUBPEL TEMPORAL FILTER RULE's calls use, and slots f - 2 and f + 2 with the grids of bbme_compose_chain_device; every grid is
 * refined by the SUBPEL RULE (K10) against (slot f, slot f +- k) into quarter-pel buffers of the context's own, allocated at first
 * use.  A colour context filters its luma planes.
 * Errors: those of the SUBPEL TEMPORAL FILTER RULE's calls: BBME_ERR_INVALID for a null context or required pointer, a neighbour
 * with only one of plane and grid, no neighbour, thr outside 1..1021, a pitch too small, a window, an output that overlaps an
 * input plane, slots outside the chain; BBME_ERR_UNSUPPORTED for the four context-level calls off a chain or beyond W0 or H0
 * 8188; BBME_ERR_STATE for those without frames and a valid bidirectional estimate.  None of these calls changes context state;
 * the statistics scratch and the quarter-pel buffers are their own (the +-1 grids share the subpel temporal filter's buffer).
 * The caller orders context-level calls that it issues on different streams.
 * bbme_wide_temporal_filter_host: the rule on the CPU, no GPU; planes[k] / grids[k] NULL = absent; out, weights (packed, CW per
 * row) and stats6 each may be NULL, not all three.
 * bbme_cells_wide_temporal_filter_device: ANY planes and grids in HBM of the context's level-0 / cell geometry; d_out rows
 * out_pitch bytes apart, d_weights rows weights_pitch uint16 apart; d_out, d_weights, d_stats6 each optional, not all three; on
 * hip_stream (NULL = the context's), no host wait.
 * bbme_wide_temporal_filter_chain_device: the composition, then the refinement launches, then ONE filter launch for slots first ..
 * first + count - 1, frame q at d_out + q out_stride.
 * bbme_get_wide_temporal_filtered_host: one slot as the chain call; synchronises; packed W0 x H0 bytes.
 * bbme_wide_temporal_filter_stats: EVERY slot of the chain from one filter launch, stats[6 f + k]; synchronises. */
int bbme_wide_temporal_filter_host(const uint8_t *const planes[4], const uint8_t *cur, int width, int height,
                                   const int16_t *const grids[4], int q4_pitch_cells, int thr, const int *window, uint8_t *out,
                                   uint16_t *weights, unsigned long long *stats6);
int bbme_cells_wide_temporal_filter_device(bbme_ctx *ctx, const uint8_t *const d_planes[4], const uint8_t *d_cur,
                                           const int16_t *const d_grids[4], int q4_pitch_cells, int thr, const int *window,
                                           uint8_t *d_out, int out_pitch, uint16_t *d_weights, int weights_pitch,
                                           unsigned long long *d_stats6, void *hip_stream);
int bbme_wide_temporal_filter_chain_device(bbme_ctx *ctx, int first, int count, int thr, uint8_t *d_out, int out_pitch,
                                           size_t out_stride, void *hip_stream);
int bbme_get_wide_temporal_filtered_host(bbme_ctx *ctx, int slot, int thr, uint8_t *out);
int bbme_wide_temporal_filter_stats(bbme_ctx *ctx, int thr, const int *window, unsigned long long *stats);

/* BGR WIDE TEMPORAL FILTER RULE (this project's own): the WIDE TEMPORAL FILTER RULE with each neighbour taken as the BGR SUBPEL
 * TEMPORAL FILTER RULE takes it.  Inputs: the W x H B,G,R frame C; the paddings pad_x, pad_y >= 0 with W0 = W + 2 pad_x and
 * H0 = H + 2 pad_y both even; up to four neighbours k = 0 .. 3 = P1, N1, P2, N2, each a colour frame X_k (one common pitch) and a
 * quarter-pel grid Q_k on C into X_k (CH x CW int16 pairs, rows q4_pitch_cells pairs apart, one pitch for all; any int16); a
 * strength thr, 1 <= thr <= 1021.  A neighbour is present when both its frame and its grid are given; at least one must be.
 * Per neighbour, each independent of the others, exactly the BGR SUBPEL TEMPORAL FILTER RULE's: the validity of s = o + (q >> 2)
 * with f = q & 3 on the padded view; the per-channel bilinear samples X'_k[j, i][c] with the single rounding (... + 8) >> 4, a tap
 * outside the frame 0 in every channel and a tap of weight 0 never read; cost = max(cost_B, cost_G, cost_R) on the ROUNDED samples;
 * w_k = 8 (thr - cost) / thr when the neighbour is valid and cost < thr, else 0.
 * With S = 8 + sum of w_k (8..40), every channel of every pixel of the cell is
 *   out[o + (j, i)] = (8 C[o + (j, i)] + sum over k of w_k X'_k[j, i] + S / 2) / S         the numerator is at most 10220.
 * The output is the UNPADDED W x H frame: cells that straddle the frame's edge write only their pixels inside the frame.  The
 * weight map is the WIDE rule's, one uint16 per cell of the padded view, w_0 | w_1 << 4 | w_2 << 8 | w_3 << 12.  Six statistics
 * over a window in cells: cells with w_k > 0 for k = 0 .. 3, the sum of all weights, the sum of |out - C| over three channels on
 * the padded view.
 * Properties.  (1) On frames with B = G = R every channel is the unpadded window of the WIDE TEMPORAL FILTER RULE's result on the
 * zero-padded plane; the map and statistics 0 .. 4 are equal and the sixth is three times the grey one.  (2) With neighbours 2 and
 * 3 absent the frame, the low byte of the map and statistics 0, 1, 4, 5 are the BGR SUBPEL TEMPORAL FILTER RULE's, bit for bit;
 * with 4 x integer grids therefore the BGR TEMPORAL FILTER RULE's.  (3) Equal frames and zero grids leave the frame unchanged,
 * every present weight 8.  (4) Exchanging two neighbours' (frame, grid) exchanges their nibbles and their counters and nothing
 * else.  (5) Any int16 is legal: s is computed in 32 bits, and no byte outside the frames is ever read.
 * WHAT IT BUYS.  PSNR gain in dB of the filtered middle frame of five over the noisy one, worst channel, interior only, one
 * independent texture per channel, true quarter-pel grids, over two sizes and three noise levels
 * (tests/test_wide_temporal_filter_bgr_cpu.py holds these and the floors 1.0 / 1.0 dB, for the tiles 0.6 / 0.4 dB):
 *     motion per frame (quarter pels)       two-sided +-1    two-sided +-2    one-sided +1     one-sided +1, +2
 *     (4, 0), (8, -8)                       +4.28..+4.51     +6.40..+6.79     +2.61..+2.83     +4.28..+4.60
 *     (2, 2), (6, -2), (10, 6), (14, -10)   +5.24..+6.68     +7.10..+8.12     +3.59..+4.20     +5.02..+5.59
 *     (1, 3), (5, -7)                       +5.29..+6.21     +6.87..+9.30     +3.44..+3.87     +5.30..+6.40
 *     2x2 tiles of four motions             +4.94..+6.34     +6.67..+7.43     +3.01..+3.88     +4.01..+4.76
 * On a CHAIN context with its own fields the grids are those the WIDE TEMPORAL FILTER RULE's context calls use -- the +-1 grids of
 * the subpel temporal filter, the +-2 grids composed, all refined by the SUBPEL RULE (K10) on the LUMA planes into the buffers the
 * grey wide calls use -- and ONE filter launch then reads only the stored colour (the COLOUR STORE above).
 * Errors: the union of the wide calls' and the BGR subpel calls'.  BBME_ERR_INVALID for a null context or required pointer,
 * bgr_pitch or out_pitch < 3 W, an out_stride below one frame when count > 1, q4_pitch_cells or weights_pitch < CW, a neighbour
 * with only one of frame and grid, no neighbour, thr outside 1..1021, a bad window, an output that overlaps an input frame, slots
 * outside the chain; BBME_ERR_UNSUPPORTED for the three context-level calls off a chain or beyond W0 or H0 8188; BBME_ERR_STATE
 * for those without frames and a valid bidirectional estimate, or when a slot the call reads has no stored colour.  None of these
 * calls changes context state; the statistics scratch is their own, the quarter-pel buffers are those of the grey wide calls.
 * bbme_wide_temporal_filter_bgr_host: the rule on the CPU, no GPU; packed frames of 3 W bytes a row; frames[k] / grids[k] NULL =
 * absent; out (packed), weights (packed, CW per row) and stats6 each may be NULL, not all three.
 * bbme_cells_wide_temporal_filter_bgr_device: ANY colour frames in HBM with one common pitch bgr_pitch >= 3 W and ANY grids of the
 * context's cell geometry; d_out rows out_pitch bytes apart, d_weights rows weights_pitch uint16 apart; d_out, d_weights,
 * d_stats6 each optional, not all three; on hip_stream (NULL = the context's), ordered behind the context's stream; no host wait.
 * bbme_wide_temporal_filter_bgr_chain_device: the composition and refinement launches of the grey chain call, then ONE filter
 * launch for slots first .. first + count - 1, frame q at d_out + q out_stride.
 * bbme_get_wide_temporal_filtered_bgr_host: one slot as the chain call; synchronises; packed rows of 3 W bytes.
 * bbme_wide_temporal_filter_bgr_stats: EVERY slot of the chain from one filter launch, stats[6 f + k]; synchronises. */
int bbme_wide_temporal_filter_bgr_host(const uint8_t *const frames[4], const uint8_t *cur, int width, int height, int pad_x, int pad_y,
                                       const int16_t *const grids[4], int q4_pitch_cells, int thr, const int *window, uint8_t *out,
                                       uint16_t *weights, unsigned long long *stats6);
int bbme_cells_wide_temporal_filter_bgr_device(bbme_ctx *ctx, const uint8_t *const d_frames[4], const uint8_t *d_cur, int bgr_pitch,
                                               const int16_t *const d_grids[4], int q4_pitch_cells, int thr, const int *window,
                                               uint8_t *d_out, int out_pitch, uint16_t *d_weights, int weights_pitch,
                                               unsigned long long *d_stats6, void *hip_stream);
int bbme_wide_temporal_filter_bgr_chain_device(bbme_ctx *ctx, int first, int count, int thr, uint8_t *d_out, int out_pitch,
                                               size_t out_stride, void *hip_stream);
int bbme_get_wide_temporal_filtered_bgr_host(bbme_ctx *ctx, int slot, int thr, uint8_t *out);
int bbme_wide_temporal_filter_bgr_stats(bbme_ctx *ctx, int thr, const int *window, unsigned long long *stats);

/* GLOBAL MOTION RULE (this project's own; the reference has no parametric motion): the dominant motion of a cell grid as a
 * translation or an affine model, and the cells that follow it.  Inputs: a grid Q of CH x CW int16 (dx, dy), CH = H0 / 2,
 * CW = W0 / 2, in GRID UNITS of 1 / unit pixel (unit = 1: integer cells; unit = 4: quarter-pel cells "4 v + q"); optionally an
 * exclusion mask E, one byte per cell (rows exclude_pitch bytes apart), non-zero = excluded -- a consistency mask can be fed as it
 * is --; a window {cx0, cy0, cw, ch} IN CELLS (NULL = all cells).  Any int16 values are allowed.
 * Coordinates are HALF PIXELS FROM THE PLANE CENTRE, so that all of them are integers: cell (cx, cy) lies at X = 4 cx + 2 - W0,
 * Y = 4 cy + 2 - H0, pixel (x, y) at X = 2 x + 1 - W0, Y = 2 y + 1 - H0; they stay plane-centred whatever the window is.
 * A MODEL is six int32 in Q16, m0..m2 for u and m3..m5 for v: pu = m0 + m1 X + m2 Y and pv = m3 + m4 X + m5 Y in 64-bit
 * integers; m0 and m3 are in grid units, the slopes in grid units per half pixel.
 * Histogram part.  Over the window's cells that E does not exclude, two histograms of BBME_GM_BINS = 2048 uint32 bins, hist[b] for
 * dx and hist[2048 + b] for dy, bin(v) = clamp(v, -1024, 1023) + 1024.  n = the sum of one histogram; the MEDIAN of a component is
 * the smallest bin whose cumulative count is >= (n + 1) >> 1, minus 1024, and 0 when n = 0.
 * Moments part, under a model and a tolerance tol_q16 (0 .. 2^40).  A cell is class BBME_GM_EXCLUDED if E excludes it; otherwise
 * r = |(dx << 16) - pu| + |(dy << 16) - pv| in 64 bits and the class is BBME_GM_INLIER if r <= tol_q16, else BBME_GM_OUTLIER.  The
 * map is one class byte per cell, for EVERY cell of the grid.  The sixteen words, over the WINDOW's cells, are 64-bit integers:
 *   [0] n0, [1] n1, [2] n2 (cells per class), [3] the sum of r over the inliers, and over the inliers [4] sum X, [5] sum Y,
 *   [6] sum XX, [7] sum XY, [8] sum YY, [9] sum dx, [10] sum dy, [11] sum X dx, [12] sum Y dx, [13] sum X dy, [14] sum Y dy,
 *   [15] sum (dx^2 + dy^2).
 * They are exact two's-complement sums (|X|, |Y| < 2^13, a product below 2^28, r below 2^47; up to 2^24 cells), word 3 as long as
 * n0 tol_q16 < 2^63; beyond that it is the sum modulo 2^64.  Hence BBME_ERR_UNSUPPORTED for W0 or H0 > 8188.
 * Solve part (host code, one function for the GPU route and the CPU route, so both get the same model from the same words).
 * Translation: m0 = [9] / n0, m3 = [10] / n0, slopes 0.  Affine: least squares of dx and of dy on (1, X, Y) over the inliers, in
 * double from the centred scatter: with n = n0, xm = [4] / n, ym = [5] / n, Sxx = [6] - [4] xm, Sxy = [7] - [4] ym,
 * Syy = [8] - [5] ym, Sxu = [11] - [4] um (um = [9] / n) and likewise Syu, Sxv, Syv, D = Sxx Syy - Sxy Sxy:
 * a1 = (Sxu Syy - Syu Sxy) / D, a2 = (Syu Sxx - Sxu Sxy) / D, a0 = um - a1 xm - a2 ym (Cramer's rule), no fused multiply-add.
 * The affine model is used only if n0 >= 3, Sxx > 0, Syy > 0 and D > Sxx Syy / 2^20; otherwise the translation is.  Each parameter
 * is llrint(value * 65536) (half to even) saturated to int32.  n0 = 0 gives the zero model.  Every moment stays below 2^53.
 * Estimate.  iterations in 0..8.  The histogram; n = 0: the model is zero.  Otherwise model = (median_x << 16, 0, 0,
 * median_y << 16, 0, 0).  Then `iterations` times: moments(model, tol_q16); stop if n0 = 0; model = solve(kind).  A last moments
 * pass under the final model gives the sixteen words and the map.
 * Limit: the start is the component-wise median.  When independently moving cells outnumber, in one component's histogram, the
 * spread of a strongly zooming or rotating background, the median starts on them and the fit can stay there (README.md).
 * Errors: BBME_ERR_INVALID for a null context or required pointer, a pair out of range, `which` not 0 or 1, `kind` not one of the
 * two, tol_q16 outside 0..2^40, iterations outside 0..8, unit not 1 or 4, a pitch < CW, a window as for the consistency rule;
 * BBME_ERR_UNSUPPORTED beyond 8188; BBME_ERR_STATE for the context's own calls exactly as bbme_subpel_device (frames, cells of
 * `which`) and, with mask_tol >= 0, as bbme_consistency_stats (a valid pair of fields).  None of these calls changes context state
 * (grids, memo, flow, cells, backward cells, captured graphs, colour store); their scratch buffers are the context's own and
 * independent of the other getters'.  All work on single, batched and chain contexts and in direction BACKWARD.
 * bbme_vector_histogram_host / bbme_global_moments_host / bbme_global_motion_solve_host / bbme_global_motion_host: the parts and
 * the whole estimate on the CPU, no GPU, on a packed cells_h x cells_w grid; exclude may be NULL; map (packed) and words16 each
 * may be NULL, not both (bbme_global_motion_host: model is required, words16 and map are optional).
 * bbme_cells_vector_histogram_device: ANY grid in HBM of the context's cell geometry, rows cells_pitch_cells int16 pairs apart;
 * d_hist (4096 uint32) is zeroed and filled on hip_stream (NULL = the ctx stream; another stream is first ordered behind it); no
 * host wait; needs no estimate and no scratch.
 * bbme_cells_global_moments_device: the same for the moments; d_map (rows map_pitch bytes apart) and d_words16 each may be null,
 * not both.  Launches with d_words16 share one scratch buffer per context: the caller orders those it issues on different streams.
 * bbme_global_motion: the estimate of EVERY pair of the context, one launch per step over all pairs with a device table of
 * models; models[6 p + k], words[16 p + k].  which = 0: the current level-0 cells, which = 1: the backward cells; subpel = 1
 * refines them first as bbme_subpel_device does and the grid unit is 4, else 1; mask_tol >= 0 excludes the cells that the
 * CONSISTENCY RULE of (which, mask_tol) does not call consistent, mask_tol < 0 excludes none.  It SYNCHRONISES AT EVERY STEP: the
 * 16 KB of counts per pair come down once and 128 bytes per pair after each moments pass, the solve runs on the host.
 * bbme_get_global_motion_map_host: the class map of `pair` under `model` for the same selection of cells; synchronises; packed
 * CH x CW bytes. */
enum { BBME_GM_TRANSLATION = 0, BBME_GM_AFFINE = 1 };
enum { BBME_GM_INLIER = 0, BBME_GM_OUTLIER = 1, BBME_GM_EXCLUDED = 2 };
enum { BBME_GM_BINS = 2048 };
int bbme_vector_histogram_host(const int16_t *cells, int cells_w, int cells_h, const uint8_t *exclude, int exclude_pitch,
                               const int *window, uint32_t *hist);
int bbme_global_moments_host(const int16_t *cells, int cells_w, int cells_h, const uint8_t *exclude, int exclude_pitch,
                             const int32_t *model, long long tol_q16, const int *window, uint8_t *map, long long *words16);
int bbme_global_motion_solve_host(const long long *words16, int kind, int32_t *model);
int bbme_global_motion_host(const int16_t *cells, int cells_w, int cells_h, const uint8_t *exclude, int exclude_pitch, int kind,
                            long long tol_q16, int iterations, const int *window, int32_t *model, long long *words16, uint8_t *map);
int bbme_cells_vector_histogram_device(bbme_ctx *ctx, const int16_t *d_cells, int cells_pitch_cells, const uint8_t *d_exclude,
                                       int exclude_pitch, const int *window, uint32_t *d_hist, void *hip_stream);
int bbme_cells_global_moments_device(bbme_ctx *ctx, const int16_t *d_cells, int cells_pitch_cells, const uint8_t *d_exclude,
                                     int exclude_pitch, const int32_t *model, long long tol_q16, const int *window, uint8_t *d_map,
                                     int map_pitch, long long *d_words16, void *hip_stream);
int bbme_global_motion(bbme_ctx *ctx, int which, int subpel, int kind, long long tol_q16, int iterations, int mask_tol,
                       const int *window, int32_t *models, long long *words);
int bbme_get_global_motion_map_host(bbme_ctx *ctx, int pair, int which, int subpel, int mask_tol, const int32_t *model,
                                    long long tol_q16, uint8_t *map);

/* GLOBAL COMPENSATION RULE (this project's own): the frame compensated for a model's motion alone, pixel by pixel, and its
 * residual statistics.  Inputs: two packed planes I1 and I2 of W0 x H0 bytes (I1 for the statistics only), a model of the GLOBAL
 * MOTION RULE and its grid unit (1 or 4).  For pixel (x, y) with its X, Y of that rule: d = (pu, pv);
 * q = (d (4 / unit) + 32768) >> 16, the arithmetic shift in 64 bits: the displacement in quarter pels; i = q >> 2, f = q & 3,
 * s = (x, y) + i.  The pixel is COMPENSATED when every tap of non-zero weight lies in the plane: 0 <= s.x, s.x + 1 + (fx != 0) <= W0,
 * 0 <= s.y and s.y + 1 + (fy != 0) <= H0; it is then the SUBPEL RULE's sample of I2 at s with the fractions f.  Otherwise it gets
 * `fill` (0..255) and counts as skipped.  No byte outside the plane is read.
 * Statistics: the four of the SUBPEL COMPENSATION RULE -- sse, sad, pixels, skipped against I1 over a window {x0, y0, w, h} in
 * PIXELS (NULL = the whole plane) --, exact and independent of `fill`.
 * Property.  With a whole-pixel translation model (m0 = tx unit << 16, m3 = ty unit << 16, slopes 0), out[y][x] =
 * I2[y + ty][x + tx] wherever that lies in the plane.
 * Errors: as for the SUBPEL COMPENSATION RULE's calls, with unit not 1 or 4 BBME_ERR_INVALID; the context's own calls need frames
 * only (BBME_ERR_STATE without; no estimate).  No call changes context state.
 * bbme_global_compensate_host: the rule on the CPU, no GPU, on packed width x height planes (both even); image1 may be NULL without
 * statistics; out (packed) and stats4 each may be NULL, not both.
 * bbme_cells_global_compensate_device: ANY packed planes in HBM of the context's level-0 geometry; d_image1 may be null without
 * d_stats4; d_out (rows out_pitch bytes apart) and d_stats4 each may be null, not both; on hip_stream as above; no host wait.
 * Launches with d_stats4 share one scratch buffer per context: the caller orders those it issues on different streams.
 * bbme_global_compensate_device: the context's own planes of `pair`: which = 0 predicts image 1 from image 2 (in direction BACKWARD
 * the planes exchange as for every plane-reading call), which = 1 image 2 from image 1.  On a chain the planes are slots pair and
 * pair + 1.  A colour context compensates its luma planes.
 * bbme_get_global_compensated_host: the same; synchronises; the packed padded W0 x H0 plane.
 * bbme_global_compensation_error: EVERY pair from one launch under its own model, models[6 p + k], stats[4 p + k]; synchronises. */
int bbme_global_compensate_host(const uint8_t *image1, const uint8_t *image2, int width, int height, const int32_t *model, int unit,
                                int fill, const int *window, uint8_t *out, unsigned long long *stats4);
int bbme_cells_global_compensate_device(bbme_ctx *ctx, const uint8_t *d_image1, const uint8_t *d_image2, const int32_t *model, int unit,
                                        int fill, const int *window, uint8_t *d_out, int out_pitch, unsigned long long *d_stats4,
                                        void *hip_stream);
int bbme_global_compensate_device(bbme_ctx *ctx, int pair, int which, const int32_t *model, int unit, int fill, uint8_t *d_out,
                                  int out_pitch, void *hip_stream);
int bbme_get_global_compensated_host(bbme_ctx *ctx, int pair, int which, const int32_t *model, int unit, int fill, uint8_t *out);
int bbme_global_compensation_error(bbme_ctx *ctx, int which, const int32_t *models, int unit, const int *window,
                                   unsigned long long *stats);

/* BGR GLOBAL COMPENSATION RULE (this project's own): the GLOBAL COMPENSATION RULE applied to the zero-padded view of a colour
 * frame; it writes the unpadded frame, as every other BGR rule does.  Inputs: two colour frames C1 and C2, each W x H pixels of
 * B,G,R with rows bgr_pitch >= 3 W bytes apart (C1 for the statistics only); pad_x and pad_y, with W0 = W + 2 pad_x and
 * H0 = H + 2 pad_y (both even, as every padded plane is); a model of the GLOBAL MOTION RULE and its unit (1 or 4); fill (0..255).
 * Output pixel (x, y) of the frame lies at padded position (x + pad_x, y + pad_y); its X, Y are 2 (x + pad_x) + 1 - W0 and
 * 2 (y + pad_y) + 1 - H0, which equal 2 x + 1 - W and 2 y + 1 - H: THE MODEL DOES NOT DEPEND ON THE PADDING.  q, i and f are exactly
 * as in the grey rule, in 64 bits; s = (x + pad_x, y + pad_y) + i.  The pixel is COMPENSATED under the grey rule's condition on the
 * padded plane W0 x H0; every channel c is then the SUBPEL RULE's sample, with its single rounding (... + 8) >> 4, of channel c at
 * s with the fractions f, where a tap whose frame coordinates lie outside [0, W) x [0, H) reads 0 -- the zero border of the luma
 * planes -- and a tap of weight 0 is never read.  A pixel that is not compensated gets `fill` in all three channels and counts as
 * skipped.  No byte outside the frames' W x H pixels is read.
 * Statistics: four words {sse, sad, pixels, skipped} against C1 over a window {x0, y0, w, h} in FRAME pixels (NULL = the whole
 * frame): sse and sad are summed over the three channels, pixels and skipped count pixels (the mirrors derive
 * mse = sse / (3 pixels) and psnr from it); exact and independent of `fill`.
 * Properties.  On B = G = R frames every channel of the output is the unpadded crop of the grey rule's output on pad_zero(grey),
 * sse and sad are three times the grey statistics over the same window, pixels and skipped are equal.  With pads of 0 each channel
 * is the grey rule on that channel.  With a whole-pixel translation model, out[y][x] = C2[y + ty][x + tx] wherever that lies in
 * the padded view (0 in its border).  The identity model returns C2.
 * Errors: as for the grey rule's calls, the window inside the frame; in addition BBME_ERR_INVALID for bgr_pitch or out_pitch < 3 W,
 * for a frame_stride or out_stride below one frame when count > 1, and for count outside 1..BBME_GC_MAX_FRAMES; BBME_ERR_STATE
 * when stored colour is asked for and a frame has none (a grey setter withdraws it); BBME_ERR_UNSUPPORTED for W0 or H0 > 8188.  No
 * call changes context state.  All work on single, batched and chain contexts.
 * bbme_global_compensate_bgr_host: the rule on the CPU, no GPU; bgr1 may be NULL without statistics; out (rows out_pitch bytes
 * apart) and stats4 each may be NULL, not both.
 * bbme_cells_global_compensate_bgr_device: ANY colour frames in HBM of the context's frame size and a common bgr_pitch: `count`
 * frames (1..BBME_GC_MAX_FRAMES), frame_stride bytes apart in both inputs, from ONE launch; models holds 6 count int32 ON THE HOST,
 * frame k under models[6 k ..] (for count > 1 they are copied to a device table on hip_stream, as bbme_global_compensation_error
 * copies its own); d_bgr1 may be null without d_stats4; d_out (rows out_pitch, frames out_stride bytes apart) and d_stats4
 * (4 count words, frame k at 4 k) each may be null, not both; the output must not overlap an input.  On hip_stream (NULL = the ctx
 * stream; another stream is first ordered behind it); no host wait.  Launches with d_stats4 share one scratch buffer per context and
 * launches with count > 1 one table: the caller orders those it issues on different streams.
 * bbme_global_compensate_bgr_device: the stored colour of `pair` (the COLOUR STORE): which = 0 predicts frame 1 from frame 2 (in
 * direction BACKWARD the frames exchange, as the planes of bbme_global_compensate_device do), which = 1 frame 2 from frame 1.  On a
 * chain the frames are slots pair and pair + 1.
 * bbme_get_global_compensated_bgr_host: the same; synchronises; packed rows of 3 W bytes.
 * bbme_global_compensation_error_bgr: EVERY pair from one launch under its own model, models[6 p + k], stats[4 p + k]; every pair
 * needs its stored colour; synchronises. */
enum { BBME_GC_MAX_FRAMES = 32 };
int bbme_global_compensate_bgr_host(const uint8_t *bgr1, const uint8_t *bgr2, int width, int height, int bgr_pitch, int pad_x, int pad_y,
                                    const int32_t *model, int unit, int fill, const int *window, uint8_t *out, int out_pitch,
                                    unsigned long long *stats4);
int bbme_cells_global_compensate_bgr_device(bbme_ctx *ctx, const uint8_t *d_bgr1, const uint8_t *d_bgr2, int bgr_pitch, size_t frame_stride,
                                            int count, const int32_t *models, int unit, int fill, const int *window, uint8_t *d_out,
                                            int out_pitch, size_t out_stride, unsigned long long *d_stats4, void *hip_stream);
int bbme_global_compensate_bgr_device(bbme_ctx *ctx, int pair, int which, const int32_t *model, int unit, int fill, uint8_t *d_out,
                                      int out_pitch, void *hip_stream);
int bbme_get_global_compensated_bgr_host(bbme_ctx *ctx, int pair, int which, const int32_t *model, int unit, int fill, uint8_t *out);
int bbme_global_compensation_error_bgr(bbme_ctx *ctx, int which, const int32_t *models, int unit, const int *window,
                                       unsigned long long *stats);

/* BGR COMPENSATION RULE (this project's own; MF::draw_MVimage, motion_framework.cpp:887-905, is grey): the SUBPEL COMPENSATION RULE
 * applied to the zero-padded view of a colour frame; it writes the unpadded frame, as every other BGR rule does.  It is the colour
 * form of per-cell motion compensation, along integer cells or along quarter-pel cells.
 * Inputs: two colour frames C1 and C2, each W x H pixels of B,G,R with rows bgr_pitch >= 3 W bytes apart (C1 for the statistics
 * only); pad_x and pad_y, with W0 = W + 2 pad_x and H0 = H + 2 pad_y (both even, as every padded plane is); a grid of CH x CW int16
 * pairs, CH = H0 / 2, CW = W0 / 2, rows pitch_cells >= CW pairs apart; unit (1 or 4); fill (0..255).  With unit 4 the grid holds
 * quarter-pel vectors as the bbme_subpel_* calls write them, (qx, qy) = Q[cy][cx].  With unit 1 it holds integer cells G and
 * (qx, qy) = 4 G[cy][cx] computed in 32 bits: any int16 is allowed and 4 G need not fit int16, which is why the unit exists.
 * Cell.  For cell (cx, cy) of the padded plane, o, i, f and s are exactly those of the SUBPEL COMPENSATION RULE, and the cell is
 * COMPENSATED under that rule's condition on the W0 x H0 plane: 0 <= s.x, s.x + 2 + (fx != 0) <= W0, 0 <= s.y and
 * s.y + 2 + (fy != 0) <= H0.
 * Pixels.  Each of the cell's four pixels lies at frame coordinates o + (j, k) - (pad_x, pad_y); a pixel inside [0, W) x [0, H) is
 * written and the others are not: with an odd pad a cell straddles the frame's edge.  A compensated cell's pixel takes, in every
 * channel, the SUBPEL RULE's sample of that channel at s + (j, k) with the fractions f and the single rounding (... + 8) >> 4, where
 * a tap whose frame coordinates lie outside the frame reads 0 -- the zero border of the luma planes -- and a tap of weight 0 is
 * never read.  A skipped cell's pixels get `fill` in all three channels.  No byte outside the frames' W x H pixels is read and no
 * byte outside the output's W x H pixels is written.
 * Statistics: four words {sse, sad, pixels, skipped} against C1 over a window {x0, y0, w, h} in FRAME pixels (NULL = the whole
 * frame): sse and sad are summed over the three channels of the window pixels of compensated cells, pixels counts those pixels and
 * skipped the window pixels of skipped cells (the mirrors derive mse = sse / (3 pixels) and psnr from it, as for the BGR GLOBAL
 * COMPENSATION RULE); all four are exact 64-bit integers and do not depend on `fill`.
 * Properties.  On B = G = R frames every channel of the output is the unpadded crop of bbme_subpel_compensate_host on
 * pad_zero(grey) and, with unit 1, of the integer compensation rule at level 0 with block 2 and grid_block 2; sse and sad are three
 * times the grey figures over the same window, pixels and skipped are equal.  With pads of 0 each channel is the grey rule on that
 * channel.  Unit 1 on G equals unit 4 on 4 G wherever 4 G fits int16.  A zero grid returns C2, and its statistics are the plain
 * frame difference.
 * Errors: as the SUBPEL COMPENSATION RULE's and the BGR GLOBAL COMPENSATION RULE's: BBME_ERR_INVALID for a null context or required
 * pointer, a pair out of range, `which` not 0 or 1, unit not 1 or 4, a fill outside 0..255, bgr_pitch or out_pitch < 3 W,
 * pitch_cells < CW, a window not inside the frame, an odd W0 or H0 on the host call, a d_out of bbme_cells_compensate_bgr_device
 * that overlaps an input frame; BBME_ERR_STATE where stored colour is asked for and a frame has none (a grey setter withdraws it),
 * and exactly as bbme_subpel_device for the cells (either unit); for the context's own calls BBME_ERR_UNSUPPORTED beyond 8188.  No
 * call changes context state (grids, memo, flow, cells, backward cells, captured graphs, colour store).  All work on single, batched
 * and chain contexts.
 * bbme_compensate_bgr_host: the rule on the CPU, no GPU; bgr1 may be NULL without stats4; out (rows out_pitch bytes apart) and
 * stats4 each may be NULL, not both.  It has no size limit of its own.
 * bbme_cells_compensate_bgr_device: ANY colour frames of the context's frame size (a common bgr_pitch) and ANY grid in HBM of the
 * context's cell geometry, grid rows pitch_cells int16 pairs apart (bbme_subpel_device's strided output can be fed straight in);
 * no frames set and no estimate needed; d_bgr1 may be null without d_stats4; d_out and d_stats4 each may be null, not both.  On
 * hip_stream (NULL = the ctx stream; another stream is first ordered behind it); no host wait.  Launches with d_stats4 share one
 * scratch buffer per context: the caller orders those it issues on different streams.
 * bbme_compensate_bgr_device: the stored colour of `pair` (the COLOUR STORE).  With unit 4 the cells of `pair` are refined on the
 * LUMA planes (bbme_subpel_device's `which`) into the quarter-pel buffer bbme_subpel_compensate_device uses, then the colour is
 * compensated from it; with unit 1 the integer cells are read as they are and no refinement is launched.  which = 0 predicts
 * frame 1 from frame 2 along the current cells (in direction BACKWARD the frames exchange, as in
 * bbme_global_compensate_bgr_device), which = 1 frame 2 from frame 1 along the backward cells of bbme_estimate_bidirectional.  On a
 * chain the frames are slots pair and pair + 1.  The caller orders calls for the same pair that it issues on different streams.
 * bbme_get_compensated_bgr_host: the same; synchronises; packed rows of 3 W bytes.
 * bbme_compensation_error_bgr: EVERY pair of the context, stats[4 p + k], from at most one refinement launch (unit 4; none with
 * unit 1) and one compensation launch over all pairs; every pair needs its stored colour; synchronises. */
int bbme_compensate_bgr_host(const uint8_t *bgr1, const uint8_t *bgr2, int width, int height, int bgr_pitch, int pad_x, int pad_y,
                             const int16_t *grid, int pitch_cells, int unit, int fill, const int *window, uint8_t *out, int out_pitch,
                             unsigned long long *stats4);
int bbme_cells_compensate_bgr_device(bbme_ctx *ctx, const uint8_t *d_bgr1, const uint8_t *d_bgr2, int bgr_pitch, const int16_t *d_grid,
                                     int pitch_cells, int unit, int fill, const int *window, uint8_t *d_out, int out_pitch,
                                     unsigned long long *d_stats4, void *hip_stream);
int bbme_compensate_bgr_device(bbme_ctx *ctx, int pair, int which, int unit, int fill, uint8_t *d_out, int out_pitch, void *hip_stream);
int bbme_get_compensated_bgr_host(bbme_ctx *ctx, int pair, int which, int unit, int fill, uint8_t *out);
int bbme_compensation_error_bgr(bbme_ctx *ctx, int which, int unit, const int *window, unsigned long long *stats);

/* ---- single stages, for parity tests against the reference's private methods (single-pair contexts only) -------- */

/* copyMVs (:828-843) + calcLevelBM (:226-244) of one level.  Leaves that level's MV
 * grid at block size block_size[level]. */
int bbme_stage_search(bbme_ctx *ctx, int level);
/* One regularize_MVs() sweep (:424-530) at block size `block` with lambda_multiplier
 * `mult` (lambda follows the reference's rule lambda = (B/2) * (B/block)).  `block` must
 * equal the level's current grid block size, or half of it (then divide_blocks, :845-862,
 * is applied first). */
int bbme_stage_regularize(bbme_ctx *ctx, int level, int block, int mult);
/* Current MV grid of a level, sampled at `block` (<= current grid block size), as
 * int16 (dx,dy) per block, row-major (height/block rows x width/block cols). */
int bbme_stage_get_mvs(bbme_ctx *ctx, int level, int block, int16_t *mvs);
/* Overwrite a level's MV grid at block size `block` (makes it the current grid). */
int bbme_stage_set_mvs(bbme_ctx *ctx, int level, int block, const int16_t *mvs);
/* copy_to_all_pixels (:815-826) on level 0 after its last divide: fills the dense field. */
int bbme_stage_expand(bbme_ctx *ctx);
/* Raw counters of the last sweep (diagnostic, 16 words): [3] safety-net passes, [4] blocks
 * re-evaluated by the solver, [5] non-convergence flag, [7] most rounds run by one wave,
 * [8] rounds summed over waves; sweeps with the SAD memo (block >= 8): [9] candidate look-ups
 * of the chain rounds, [10] of them not in the memo, [11] group passes that summed those,
 * [12] changes whose dependants' SADs were forwarded; [13] (rounds << 16 | rounds that left
 * queued blocks waiting) of the wave with the most rounds, [14] such rounds summed over waves
 * (how much of a sweep is queueing rather than a dependency chain), [15] evaluations made on flood
 * speculation that counted (sweeps the BBME_FLOOD_RULE selects).  [4] and [7..15] are only counted by
 * sweeps run through bbme_stage_regularize (hundreds of waves adding to the same words is a
 * queue at the memory side that bbme_estimate does not stand in); [3] and [5] always. */
int bbme_sweep_stats(bbme_ctx *ctx, unsigned *stats16);
/* Blocks per level that the last bbme_estimate searched again behind a speculative search (diagnostic; bbme_set_speculation):
 * counts[l] for the levels l < n of pair `pair`, 0 for a level whose search was not speculative (the coarsest, levels below the
 * speculation threshold or searched by the generic kernel, a profiled pass, speculation off).  Waits for the ctx stream. */
int bbme_fixup_counts(bbme_ctx *ctx, int pair, unsigned *counts, int n);
/* Fix-up passes the last sweep needed after its first full pass (diagnostic). */
int bbme_last_sweep_passes(bbme_ctx *ctx, int *passes);

/* Times (ms, HIP events on the ctx stream) of the last bbme_estimate when profiling
 * was enabled: total, and the sum over levels of search / regulariser / expand kernels. */
int bbme_set_profiling(bbme_ctx *ctx, int enabled);
int bbme_get_timings(bbme_ctx *ctx, float *total_ms, float *search_ms, float *regularize_ms,
                     float *expand_ms, float *search_level0_ms);

/* Measures the chip-wide issue rate of v_qsad_pk_u16_u8 (gops[0]) and v_sad_u8 (gops[1]) in 1e9
 * wave-instructions per second (8 waves per SIMD, 8 independent chains per lane): the VALU
 * ceilings bench.py prices the search kernel against.  gops[2] / gops[3]: QSAD rate when every QSAD
 * is interleaved with one / four independent v_sad_u8 (do the two instructions overlap?). */
int bbme_probe_rates(int device, double *gops);

/* The two candidate inner loops of the search kernel, reduced to their LDS reads and SAD instructions and run at the
 * occupancy their LDS footprints allow: tabs[0] = v_qsad_pk_u16_u8 strips over one copy of the window (what k_search_fast
 * does, 6.75 KB per wave), tabs[1] = v_sad_u8 over four byte-shifted copies (27 KB per wave), in 1e12 abs-diff per second.
 * The measurement behind the choice of instruction. */
int bbme_probe_search_loops(int device, double *tabs2);

/* Dependent-chain latency of the memory operations a solver round is made of, one lane on an idle
 * chip: out[2k] = shader cycles per operation, out[2k+1] = 10 ns ticks for 256 operations, for
 * k = 0 plain load, 1 agent-scope load, 2 returning atomic, 3 agent-scope store + drain. */
int bbme_probe_latency(int device, unsigned long long *out9);

/* Checks on the device what the kernels' XCD-aware block orders assume: that workgroups b and b + 8 of a launch run on
 * the same XCD (HW_REG_XCC_ID read by 4096 workgroups).  xcds_seen = distinct XCDs, violations = workgroups whose XCD
 * differs from that of workgroup b mod 8.  Speed only -- no result depends on the placement. */
int bbme_probe_xcd(int device, int *xcds_seen, int *violations);

/* Profiling aid: launches a kernel that reads `mbytes` MiB exactly once with one aligned dword per
 * lane (the access shape of the search kernel's window staging), `repeats` times, so that the
 * FETCH_SIZE counter can be calibrated against a known byte count in the same rocprofv3 run. */
int bbme_calibrate_read(int device, unsigned mbytes, int repeats);

/* Instruction probes used by the GPU test-suite: checks v_sad_u8, v_alignbyte_b32,
 * v_qsad_pk_u16_u8 and v_sad_u16 against a scalar model on 65536 random operands, and unaligned
 * dword / dwordx2 / dwordx4 global loads against byte-assembled values.
 * mismatches[0..4] receive the number of disagreements per item, in that order. */
int bbme_selftest_isa(int device, int *mismatches);

/* ---- test hooks ------------------------------------------------------------------------------------------------------------
 * Two environment variables, read at every device allocation (allocations are rare; an estimate makes none):
 *   BBME_TEST_GUARD=1   every device allocation of n bytes becomes [4096 guard bytes][n bytes][4096 guard bytes], the guards
 *                       filled with one byte pattern (0xA5).  The library registers every live guarded allocation and scans a
 *                       buffer's guards when it is freed or replaced; damage found then is remembered until the reset below.
 *   BBME_TEST_POISON=1  a fresh data buffer -- grids, upload buffer, colour store, staging area, statistics partials, scratch,
 *                       the slack behind an uploaded table -- is filled with a second pattern (0xC7) instead of being left as
 *                       the allocator returned it.  Zeroed buffers stay zero; index lists, whose valid length is a counter's,
 *                       are left alone.
 * With neither set the library allocates exactly as it does without these hooks.
 *
 * bbme_test_guard_check waits for every device that holds a guarded allocation, downloads and scans every live guard and adds
 * the remembered damage of buffers that are gone.  live = guarded allocations alive in this process, violations = damaged guard
 * bands (two per allocation at most).  first (first_len bytes, may be 0): the first damaged band as "<what> (<n> bytes): back
 * guard, offset 5 from the payload's edge holds 0x00 (...)" -- the buffer's text as in the library's allocation errors, front or
 * back, the offset of the nearest damaged byte counted from the payload's edge (0 touches the payload), and the byte found;
 * empty when nothing is damaged. */
int bbme_test_guard_check(unsigned long long *live, unsigned long long *violations, char *first, int first_len);
/* Forgets the remembered damage of buffers that are gone (live buffers are scanned afresh by every check). */
int bbme_test_guard_reset(void);
/* The first byte of the front (back = 0) or back (back = 1) guard band of the oldest live guarded allocation whose text is `what`
 * ("work buffers": the flow field): 4096 bytes of the library's own allocation, so that a test can damage one and see the check
 * fail.  The byte at offset k from the payload's edge is byte k of a back band and byte 4095 - k of a front band.
 * BBME_ERR_UNSUPPORTED when BBME_TEST_GUARD is unset, BBME_ERR_INVALID when there is no such allocation. */
int bbme_test_guard_find(const char *what, int back, void **guard_address);

#ifdef __cplusplus
}
#endif
#endif /* BBME_H */
