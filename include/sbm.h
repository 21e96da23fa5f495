/*
 * sbm.h — C ABI of libsbm_hip.so, the MI355X (gfx950) LINE-2D matching engine.
 *
 * This is the drop-in boundary for the match() hot path of
 * ddcr/shape_based_matching.  The reference has no FFI layer: its boundary is
 * the C++ class line2Dup::Detector (line2Dup.h:257-333).  include/line2Dup.h in
 * this repository re-declares that class and implements it on top of the
 * functions below, so a reference caller (test.cpp, test_jabil.cpp) re-links
 * against this library unchanged; other hosts bind the C ABI directly
 * (INTEGRATION.md shows both).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success or a negative sbm_status, with a message available from
 * sbm_last_error() (thread-local).  One context drives one GPU; a context is
 * not thread-safe, different contexts may be used concurrently.  "host"
 * pointers are ordinary process memory, "device" pointers are HBM addresses on
 * the context's GPU (e.g. torch tensors' data_ptr()), `stream` is a
 * hipStream_t passed as void* (NULL = the context's own stream).
 *
 * Each entry point cites the reference function (file:line) it replaces.
 */
#ifndef SBM_H
#define SBM_H

#include <stdint.h>
#include "sbm_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SBM_ABI_VERSION 1

typedef enum sbm_status {
    SBM_OK = 0,
    SBM_ERR_INVALID = -1,   /* bad argument (CV_Assert / CV_Error in the reference) */
    SBM_ERR_HIP = -2,       /* HIP runtime failure or no usable GPU */
    SBM_ERR_CAPACITY = -3,  /* candidate / match buffer too small */
    SBM_ERR_STATE = -4      /* call sequence error (no templates, no pyramid, ...) */
} sbm_status;

typedef struct sbm_ctx sbm_ctx;

/* Detector constructor arguments that matter to match()
 * (line2Dup.cpp:1056-1076: pyramid_levels, T_at_level, ColorGradient::weak_threshold). */
typedef struct sbm_config {
    int32_t n_levels;
    int32_t T[SBM_MAX_LEVELS];
    float weak_threshold;
    int32_t device_id;
    int64_t max_candidates; /* capacity of the coarse-candidate and match lists; 0 = 1<<20 */
} sbm_config;

const char* sbm_last_error(void);
int sbm_abi_version(void);

int sbm_create(const sbm_config* cfg, sbm_ctx** out);
void sbm_destroy(sbm_ctx* ctx);

/* ---- templates ----------------------------------------------------------
 * Replaces the in-memory TemplatesMap the reference walks in matchClass
 * (line2Dup.h:319-321, line2Dup.cpp:1160-1172).  levels is [n_templates][n_levels]
 * (level 0 first), features is the flat array the levels index into;
 * class_idx / template_id label the emitted matches (either may be NULL:
 * class 0 / id = position).  Templates with >= 8192 features at any level are
 * rejected with SBM_ERR_INVALID (CV_Error, line2Dup.cpp:1195, :1260). */
int sbm_upload_templates(sbm_ctx* ctx, int32_t n_templates, const sbm_template_level* levels,
                         const sbm_feature* features, int64_t n_features,
                         const int32_t* class_idx, const int32_t* template_id);

/* Restrict matching to templates whose class_idx is listed (Detector::match's
 * class_ids argument, line2Dup.cpp:1124-1140).  n == 0 selects every class.  A
 * second form selects an explicit template index range [first, first+count):
 * the template shard of one GPU (reference analogue: the OpenMP loop bounds,
 * line2Dup.cpp:1169-1170). */
int sbm_select_classes(sbm_ctx* ctx, const int32_t* class_idx, int32_t n);
int sbm_select_range(sbm_ctx* ctx, int32_t first, int32_t count);

/* An explicit list of template indices (upload order) as the active set: what sbm_select_classes / sbm_select_range
 * build internally; used to shard a class selection over several GPUs. */
int sbm_select_templates(sbm_ctx* ctx, const int32_t* template_idx, int32_t n);
/* Contiguous, work-balanced shards of a template list for a rows x cols frame: the list is template_idx[0..n) (NULL:
 * every uploaded template in upload order); shard s is list[first[s] .. first[s] + count[s]).  Work = byte-adds of the
 * coarse pass (in-bounds coarsest-level features x template_positions, line2Dup.cpp:818-837). */
int sbm_partition_templates(sbm_ctx* ctx, int32_t rows, int32_t cols, const int32_t* template_idx, int32_t n,
                            int32_t n_shards, int32_t* first, int32_t* count);

/* ---- whole hot path -----------------------------------------------------
 * Detector::match (line2Dup.cpp:1078-1150) without the final std::sort /
 * std::unique: emits the pre-dedup multiset of matches in unspecified order;
 * sbm_canonicalize() applies the epilogue.  img is 8-bit, 1 or 3 interleaved
 * channels (BGR order as cv::imread gives), row stride in bytes; mask (rows x
 * cols, non-zero = keep) may be NULL.  rows/cols must satisfy the reference's
 * preconditions at every level (rows_l % T_l == 0, cols_l % T_l == 0,
 * (rows_l * cols_l) % 16 == 0; line2Dup.cpp:639, :751-752) else SBM_ERR_INVALID.
 * The host-memory entry points (sbm_match, sbm_match_batch_host*, sbm_build_pyramid, sbm_set_quantized,
 * sbm_match_templates, the stage reads) are ordered after every device entry point enqueued before them on a caller's
 * stream: the first one after such a call waits for the device. */
int sbm_match(sbm_ctx* ctx, const uint8_t* img_host, int32_t rows, int32_t cols, int32_t stride,
              int32_t channels, const uint8_t* mask_host, float threshold, sbm_match_rec* out_host,
              int64_t cap, int64_t* n_out);

/* Single-process multi-GPU form of sbm_match: one context per GPU (all holding the same templates, each with its own
 * selection -- sbm_partition_templates + sbm_select_range / sbm_select_templates), one host thread per context, the
 * frame uploaded to every GPU, the per-GPU lists concatenated on the host: the reference's OpenMP team over
 * templates with its concatenating reduction (line2Dup.cpp:1166-1170).  One process per GPU + RCCL is the other
 * multi-GPU form (sbm_comm_* below).  Several contexts on ONE GPU are allowed (tests). */
int sbm_match_sharded(sbm_ctx* const* ctxs, int32_t n_ctx, const uint8_t* img_host, int32_t rows, int32_t cols,
                      int32_t stride, int32_t channels, const uint8_t* mask_host, float threshold,
                      sbm_match_rec* out_host, int64_t cap, int64_t* n_out);

/* A batch of frames from HOST memory, pipelined (streaming API with asynchronous upload overlap; the
 * reference calls Detector::match once per frame, line2Dup.cpp:1078): the frames travel over PCIe in sub-batches of
 * `sub_batch` frames (0 = 8) on a copy stream into one of two device buffers while the kernels of the previous
 * sub-batch run; every kernel is launched once per sub-batch (as in sbm_match_batch_device); the lists arrive in a
 * pinned host block written by the last kernel.  frames[f] points to frame f (rows x stride bytes).  Results: the
 * records of frame f at out + f * cap, {n_matches, overflow} at counts + 2 * f.  _begin enqueues everything and
 * returns (uploads from memory that is not pinned are staged by the runtime and may block meanwhile); _end waits and
 * copies the lists out; one batch in flight per context.  The frames and the mask must stay mapped and unchanged
 * from _begin until _end has returned (pinned memory is read by the copy engine during that time).
 * SBM_ERR_CAPACITY if a frame has more than cap matches (its first cap records are still returned).
 * The mask, if any, is shared by the frames; the _masked forms below take one per frame. */
int sbm_match_batch_host_begin(sbm_ctx* ctx, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols,
                               int32_t stride, int32_t channels, const uint8_t* mask_host, float threshold, int64_t cap,
                               int32_t sub_batch);
int sbm_match_batch_host_end(sbm_ctx* ctx, sbm_match_rec* out_host, int32_t* counts);
int sbm_match_batch_host(sbm_ctx* ctx, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols,
                         int32_t stride, int32_t channels, const uint8_t* mask_host, float threshold,
                         sbm_match_rec* out_host, int64_t cap, int32_t* counts, int32_t sub_batch);
/* The same pipeline with one mask per frame: the mask argument of Detector::match belongs to the call (line2Dup.cpp:1078;
 * quantize() applies it at every level, :446-450), so frame f is matched under masks[f] (rows x cols bytes, non-zero =
 * keep) exactly as sbm_match(frames[f], ..., masks[f], ...) would.  A NULL entry means no mask for that frame (the
 * library supplies an all-255 one).  The masks travel with their sub-batch into a second pair of device buffers on the
 * copy stream and must stay mapped and unchanged until _end, like the frames.  sbm_match_batch_host_end and
 * sbm_match_batch_host_end_nms end either form. */
int sbm_match_batch_host_begin_masked(sbm_ctx* ctx, const uint8_t* const* frames, int32_t n_frames, int32_t rows,
                                      int32_t cols, int32_t stride, int32_t channels, const uint8_t* const* masks_host,
                                      float threshold, int64_t cap, int32_t sub_batch);
int sbm_match_batch_host_masked(sbm_ctx* ctx, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols,
                                int32_t stride, int32_t channels, const uint8_t* const* masks_host, float threshold,
                                sbm_match_rec* out_host, int64_t cap, int32_t* counts, int32_t sub_batch);

/* Optional: pin a caller-owned host buffer (hipHostRegister) so that sbm_match / sbm_build_pyramid upload frames that
 * lie inside it with one asynchronous DMA instead of the runtime's staged pageable copy (a camera loop that re-uses
 * its frame buffer: 115 instead of ~160 us per 1024 x 1024 BGR match).  Explicit by design -- the library never pins
 * memory it was merely handed: the caller must keep the range mapped until sbm_unpin_host_buffer (or sbm_destroy)
 * and must not free / re-map it while pinned.  Buffers the caller pinned itself (hipHostMalloc, hipHostRegister)
 * need neither call.  sbm_unpin_host_buffer waits for the context's stream first. */
int sbm_pin_host_buffer(sbm_ctx* ctx, const void* host_ptr, int64_t bytes);
int sbm_unpin_host_buffer(sbm_ctx* ctx, const void* host_ptr);

/* Same path with the frame already resident in HBM.  Asynchronous: enqueues
 * every kernel on `stream` and returns.  The FIRST call after a change of state (templates, template selection,
 * threshold, frame geometry, batch size) rebuilds small device tables on the context's own stream and synchronises
 * the device before it enqueues anything: warm the context up with one call before capturing `stream` into a
 * hipGraph or relying on asynchrony; steady-state calls never wait on the host and never touch another stream.  Results go to caller-provided device
 * buffers (d_out: cap records, d_count: one int32 — the number of matches,
 * which may exceed cap, in which case only cap records were stored) so the host
 * side can all-gather them over RCCL without another copy. */
int sbm_match_device(sbm_ctx* ctx, const void* d_img, int32_t rows, int32_t cols, int32_t stride,
                     int32_t channels, const void* d_mask, float threshold, void* d_out,
                     int64_t cap, void* d_count, void* stream);

/* A batch of frames of one geometry in one call (the streaming row; the reference
 * calls Detector::match once per frame, line2Dup.cpp:1078).  Frame f starts at d_imgs + f * frame_stride
 * bytes; every kernel of the path is launched once for the whole batch (the frame is a grid dimension), so
 * the per-launch cost is shared by n_frames frames.  Results of frame f: records at d_out + f * cap,
 * {n_matches, overflow} at d_counts + 2 * f (int32); a result mirror (sbm_set_result_mirror) must hold
 * n_frames * cap records and n_frames * 2 int32, laid out the same way.  The mask, if any, is shared by
 * the frames (one mask per frame: sbm_match_batch_device_masked).  Takes every geometry sbm_match_device takes with strides up to 16: T in {4, 8} on
 * level widths that are multiples of 16 through the register-only linear-memory kernel, any other stride or width
 * through the batched any-stride one (spread bytes instead of strips and bit strips).  A stride above 16:
 * SBM_ERR_INVALID for more than one frame.  Each frame's list is what sbm_match_device returns for that frame alone. */
int sbm_match_batch_device(sbm_ctx* ctx, const void* d_imgs, int64_t frame_stride, int32_t n_frames, int32_t rows,
                           int32_t cols, int32_t stride, int32_t channels, const void* d_mask, float threshold,
                           void* d_out, int64_t cap, void* d_counts, void* stream);

/* sbm_match_batch_device with one mask per frame: frame f is gradient-quantised under the mask at d_masks +
 * f * mask_stride bytes (rows x cols, non-zero = keep), as Detector::match(source_f, threshold, class_ids, mask_f)
 * (line2Dup.cpp:1078) does -- quantize() applies the mask at every level (:446-450) and pyrDown() resizes it to the next
 * level with nearest-neighbour sampling (:439), level l's mask from level l-1's, frame by frame.  Frame f's list is what
 * sbm_match_device returns for frame f under mask f.  d_masks must not be NULL.  mask_stride == 0 is exactly
 * sbm_match_batch_device with that one mask; any other stride must be >= rows * cols (SBM_ERR_INVALID otherwise).  A
 * replayed graph reads the masks from d_masks at replay time, as it reads the frames; the same pointer with another
 * stride is another graph. */
int sbm_match_batch_device_masked(sbm_ctx* ctx, const void* d_imgs, int64_t frame_stride, int32_t n_frames, int32_t rows,
                                  int32_t cols, int32_t stride, int32_t channels, const void* d_masks,
                                  int64_t mask_stride, float threshold, void* d_out, int64_t cap, void* d_counts,
                                  void* stream);

/* sbm_match_batch_device for frames that are not one block: the loop of Detector::match (line2Dup.cpp:1078) over frames
 * that lie anywhere in device memory -- separately allocated tensors, the slots of a capture ring in any order,
 * equal-sized windows cut out of larger frames.  d_frame_ptrs is a DEVICE array of n_frames 64-bit addresses; entry f is
 * the first pixel of frame f.  All frames share rows, cols, stride (bytes per row, >= cols * channels, so a window's stride
 * is its canvas's row) and channels; they may overlap, repeat, lie in different allocations and be more than 4 GiB apart.
 * d_mask_ptrs is NULL or a device array of n_frames addresses of rows x cols masks (non-zero = keep, applied as
 * sbm_match_batch_device_masked applies them); two entries may be equal, a zero entry is NOT allowed -- the caller's
 * obligation, which the host cannot check without a synchronisation.
 * The host never dereferences either table: the level-0 gradient kernels read them on `stream`, when they run.  The tables,
 * the frames and the masks must stay valid and unchanged until the call's work on the stream has finished.  A replayed
 * graph reads the tables at replay time, and its key holds the two table ADDRESSES and `flags` in place of d_imgs,
 * frame_stride, d_masks and mask_stride -- not the tables' contents: one captured graph serves a stream of batches whose
 * frames move, the caller rewriting the table (on the same stream) between replays.  The first-call rule of
 * sbm_match_device is unchanged.
 * flags: 0 or SBM_PTRS_ALIGNED4, the caller's promise that every frame pointer is a multiple of 4.  With it, stride % 4
 * == 0, cols % 64 == 0 and a frame below 0x7ff00000 bytes, the source pass of the sparse level-0 path moves whole lines
 * (sbm_get_source_form reports 2); without it the strided form runs (1).  Same results either way.  A BROKEN PROMISE IS
 * UNDEFINED BEHAVIOUR: the line form loads dwords at the addresses it is given.
 * d_out, cap, d_counts and the result mirror are laid out as for sbm_match_batch_device, and frame f's list is what
 * sbm_match_device returns for that frame alone under its mask; the context is left in the state that call leaves.
 * SBM_ERR_INVALID: NULL d_frame_ptrs, n_frames < 1, unknown flag bits, stride < cols * channels, and every geometry
 * sbm_match_batch_device refuses (a stride above 16 with more than one frame). */
#define SBM_PTRS_ALIGNED4 1
int sbm_match_batch_device_ptrs(sbm_ctx* ctx, const void* d_frame_ptrs, int32_t n_frames, int32_t rows, int32_t cols,
                                int32_t stride, int32_t channels, const void* d_mask_ptrs, int32_t flags,
                                float threshold, void* d_out, int64_t cap, void* d_counts, void* stream);

/* sbm_match_batch_device_ptrs for PLANAR frames of three channels: a [B, 3, H, W] image batch, the [3, H, W] output of a GPU
 * JPEG decoder, the three planes of a decoder or ISP surface -- matched where they lie, without an interleaving copy.
 * d_plane_ptrs is a DEVICE array of 3 * n_frames 64-bit addresses; entry 3 f + c is the first byte of channel c of frame f, and
 * channel c is what the reference sees as interleaved channel c (B, G, R for a cv::imread frame).  The order is the caller's:
 * listing the planes of an RGB tensor as (2, 1, 0) IS the BGR frame.  `stride` is the bytes per row of a plane, shared by all
 * planes of all frames, >= cols (a window of a larger [3, H, W] canvas: the canvas's W).  Planes need no alignment; they may
 * overlap, repeat (the three entries of a frame may be equal) and lie in different allocations more than 4 GiB apart.  Always
 * three channels: a gray planar frame is a frame of sbm_match_batch_device_ptrs with channels = 1.
 * d_mask_ptrs, the tables' lifetime, the graph key (the two table addresses, not their contents; a _ptrs call at the same table
 * address is another graph), d_out, cap, d_counts, the result mirror and the state the context is left in are those of
 * sbm_match_batch_device_ptrs.  Inside the context everything stays interleaved: level 1's image, and the retained copy of level
 * 0 that the sparse path and the accessors read (sbm_get_quantized_frame, sbm_match_templates) -- the source pass re-interleaves
 * the planes as it copies them.  That pass is always the strided form (sbm_get_source_form reports 1).
 * flags is reserved and must be 0.
 * SBM_ERR_INVALID: NULL d_plane_ptrs, n_frames < 1, flags != 0, stride < cols, and every geometry sbm_match_batch_device refuses
 * (a stride above 16 with more than one frame).
 * Not offered: the C++ facade (cv::Mat has no planar three-channel form), the sharded, banded and host-batch entry points, a
 * line-shaped source pass, four-channel surfaces. */
int sbm_match_batch_device_planes(sbm_ctx* ctx, const void* d_plane_ptrs, int32_t n_frames, int32_t rows, int32_t cols,
                                  int32_t stride, const void* d_mask_ptrs, int32_t flags, float threshold, void* d_out,
                                  int64_t cap, void* d_counts, void* stream);

/* hipGraph replay of an entry point's launches: the kernel sequence of a call is recorded once per distinct argument
 * tuple (stream capture) and replayed with one hipGraphLaunch.
 *   enabled = -1 (default, "auto"): sbm_match_batch_device and sbm_match_templates_device replay once the caller keeps
 *       several calls in flight (sbm_set_pipeline_depth >= 2) and an argument tuple comes back (a tuple is captured at
 *       its second sighting; up to 16 captures are kept; a caller whose tuples never repeat stays on stream launches).
 *       Why: with several streams in flight about one process in eight on the MI355X pool runs its stream launches in a
 *       slow mode (0.5 - 1.8 ms per 16-frame step instead of 0.11, kernel durations unchanged) that replay -- one host
 *       call per step -- does not have; otherwise the two measure the same.  sbm_match_device (one frame at a time)
 *       stays on stream launches: there the replayed graph is slower (74 - 85 us against 70 us on ROCm 7.2).
 *   enabled = 0: never (the opt-out; also what profiling uses).
 *   enabled = 1: always, sbm_match_device included (two branches: the fine levels' linear memories are built while the
 *       coarse-level chain runs).
 * Results are identical either way. */
int sbm_set_graph_mode(sbm_ctx* ctx, int32_t enabled);
/* How many captured graphs the context holds right now (a test / diagnostics accessor for the rule above). */
int sbm_graph_count(sbm_ctx* ctx, int32_t* n_graphs);

/* Which gradient kernel (quantizedOrientations + hysteresisGradient, line2Dup.cpp:313-404, :218-311) the match
 * entry points launch.  mode 0 (default): by launch size — the row-streaming kernel (one wave per 256-column
 * strip, registers + DPP only, no LDS / barriers) when a launch has thousands of waves of work (a batch of
 * frames), else the 16 x 64 tile kernel, which also serves the float outputs and widths that are not a multiple
 * of 4.  mode 1: always the tile kernel.  mode 2: the streaming kernel whenever the geometry allows it.
 * rows_per_wave > 0 overrides the streaming kernel's rows per work item (rounded up to even).  Results are
 * bit-identical either way; this is a tuning / test knob. */
int sbm_set_quantize_mode(sbm_ctx* ctx, int32_t mode, int32_t rows_per_wave);

/* Which coarse-pass kernel (similarity / similarity_64 + candidate scan, line2Dup.cpp:807-858, :924-984, :1199-1216) the
 * match entry points launch.  0 (default): by launch size -- one wave per (1024 positions, template, frame) for batches
 * and large template sets, four waves sharing an item's features for a single frame with a few hundred templates;
 * 1: always the four-wave kernel; 2: always the one-wave kernel.  Identical candidates either way; a test / tuning knob. */
int sbm_set_coarse_mode(sbm_ctx* ctx, int32_t mode);

/* Which form of a refinement level with T = 4 the match entry points build (and the template loop builds, once per pyramid,
 * beside response planes that the stage entry points made) and the refinement pass (similarityLocal(_64),
 * line2Dup.cpp:860-922, :986-1048) reads.  1: BIT STRIPS -- per (sub-plane, orientation, strip of 16 columns, grid row) one
 * dword, "response > 0" bits of the 16 cells | "response == 4" bits << 16; the reference's sum of response bytes {0, 3, 4}
 * is 3 #any + #exact, counted with bit-sliced carry-save counters, one wave per candidate.  0: one plane of spread bytes,
 * the response looked up per byte (rounds 2-3).  -1 (default): the process default (bit strips unless SBM_LOCAL_BITS=0).
 * Levels with another T, or whose grid width is not a multiple of 16 cells, use the byte form either way.  Identical
 * matches; a test / tuning knob. */
int sbm_set_refine_bits(sbm_ctx* ctx, int32_t mode);

/* Which candidate a workgroup of the refinement pass (similarityLocal(_64) + the loop at line2Dup.cpp:1221-1293) takes.
 * 0: a grid of (frames x slots), every frame's candidates walked by that frame's slots; 2: the candidates of up to 64
 * frames as ONE frame-major list walked by the whole grid (the workgroups running together stay on one or two frames,
 * whose linear memories then stay in the L2s); -1 (default): 2 once the batch's finest-level planes exceed the L2s
 * together (32 MiB), else 0.  Identical matches either way; a test / tuning knob. */
int sbm_set_refine_order(sbm_ctx* ctx, int32_t order);

/* Hint: how many batches the caller keeps in flight on this GPU at the same time (through other contexts and
 * streams; bench.py runs three).  1 (default): every launch is sized for its own latency -- all its work items resident
 * at once.  >= 2: launches are sized for throughput -- the row-streaming gradient kernel takes fewer, longer work items
 * (less warm-up work in total), down to one wave per SIMD of the chip ("Rows per work item"), at about
 * 1.3x the latency of a batch alone.
 * Results are identical either way. */
int sbm_set_pipeline_depth(sbm_ctx* ctx, int32_t batches_in_flight);

/* The sparse level-0 gradient launch of a batch call runs a frame of few coarse candidates from a list of its working items
 * (sbm_get_sparse_list).  rows_per_item: the rows per work item of the grid those lists are made on.  -1 (default): the process
 * default -- SBM_SPARSE_LIST_HS in the environment, else chosen like the rows per item of a whole-level launch from the frames of
 * the call when several batches are in flight (sbm_set_pipeline_depth >= 2), and the launch's own rows per item otherwise and
 * wherever sbm_set_quantize_mode has set those; 0: always the launch's own; > 0: that many (rounded up to even).  A frame without
 * a list keeps the launch's own grid.  Identical results; a test / tuning knob. */
int sbm_set_sparse_list_rows(sbm_ctx* ctx, int32_t rows_per_item);

/* Optional second destination for the results of sbm_match_device /
 * sbm_match_templates: every match record (up to the call's cap) and the final
 * {n_matches, overflow} pair are ALSO stored, with plain stores from the last
 * kernel, at these device-visible addresses — typically pinned host memory
 * (hipHostMalloc / torch pin_memory), so the match list reaches the host with
 * no copy-engine operation after the kernels.  Pass NULL, NULL to disable.  The
 * mirror must hold cap records / two int32 and outlive the calls using it. */
int sbm_set_result_mirror(sbm_ctx* ctx, void* mirror_out, void* mirror_count);

/* ---- multi-GPU: template shards + one RCCL exchange step -------------------
 * The reference's only parallelism is the OpenMP loop over templates whose
 * per-thread match vectors are concatenated by a reduction
 * (line2Dup.cpp:1166-1170).  Analogue: one context (process) per GPU, each with
 * a template range (sbm_select_range), and ONE collective per frame: an
 * ncclAllGather over xGMI of the per-rank lists, issued by the library on the
 * same stream as the kernels.  librccl is resolved with dlopen on first use.
 *
 *   sbm_comm_unique_id   rank 0: 128-byte id to hand to every rank (any transport)
 *   sbm_comm_init        every rank: join the communicator on the context's GPU
 *   sbm_match_device_sharded
 *        d_local    : SBM_SHARD_HEADER_BYTES + cap * 24 bytes, this rank's list:
 *                     int32 {n_matches, overflow, 0, 0} then the records
 *        d_gathered : world * (that size), all ranks' lists in rank order
 *        gathered_mirror : optional device-visible copy of d_gathered (pinned host)
 */
#define SBM_COMM_ID_BYTES 128
#define SBM_SHARD_HEADER_BYTES 16
int sbm_comm_unique_id(void* id_out);
int sbm_comm_init(sbm_ctx* ctx, int32_t world, int32_t rank, const void* id);
int sbm_comm_destroy(sbm_ctx* ctx);
/* Size of the context's communicator as RCCL reports it (ncclCommCount): what a launcher records as "ranks seen". */
int sbm_comm_count(sbm_ctx* ctx, int32_t* n_ranks);
/* The template loop alone (sbm_match_templates_device: matchClass over the selected templates on the resident pyramid,
 * line2Dup.cpp:1160-1297) followed by the same exchange step as sbm_match_device_sharded: d_local = 16-byte header
 * {n_matches, overflow, 0, 0} + cap records, d_gathered = world such shards in rank order.  The sharded form of
 * BASELINE configs 3 and 4 (template ranges over the ranks, pyramid resident on each). */
int sbm_match_templates_device_sharded(sbm_ctx* ctx, float threshold, void* d_local, int64_t cap, void* d_gathered,
                                       void* gathered_mirror, void* stream);
int sbm_match_device_sharded(sbm_ctx* ctx, const void* d_img, int32_t rows, int32_t cols, int32_t stride,
                             int32_t channels, const void* d_mask, float threshold, void* d_local,
                             int64_t cap, void* d_gathered, void* gathered_mirror, void* stream);
/* The same exchange for a batch of frames (sbm_match_batch_device + one ncclAllGather of the whole shard):
 *   d_local : header = n_frames * 8 bytes rounded up to 16 ({n_matches, overflow} int32 pairs), then
 *             n_frames blocks of cap records; d_gathered: world such shards in rank order. */
int sbm_match_batch_device_sharded(sbm_ctx* ctx, const void* d_imgs, int64_t frame_stride, int32_t n_frames,
                                   int32_t rows, int32_t cols, int32_t stride, int32_t channels,
                                   const void* d_mask, float threshold, void* d_local, int64_t cap,
                                   void* d_gathered, void* gathered_mirror, void* stream);

/* Build-sharded step (round 3): the gradient stage is sharded too.  The reference builds the pyramid serially
 * (line2Dup.cpp:1084-1120) and parallelises only the template loop (:1166-1170); with the pyramid replicated on every
 * rank a step cannot scale past (build + loop) / build.  Here rank r of a world of n computes ROW BAND r of every
 * level's orientation map (quantizedOrientations + hysteresisGradient of rows [r, r+1) * rows_l / n, plus the halo
 * rows the next level's band needs through the fused cv::pyrDown), one grouped in-place ncclAllGather over xGMI
 * assembles the maps on every rank (1 byte per pixel and level: 1.25 MiB per 1024 x 1024 frame), every rank builds
 * the linear memories from the assembled maps and matches its template range (sbm_select_range), and the per-rank
 * match lists are gathered as in sbm_match_batch_device_sharded (same d_local / d_gathered layout).
 * Needs rows_l % n == 0 with an even quotient at every level, cols % 4 == 0.  The assembled maps are bit for bit the
 * maps of sbm_match_batch_device (a band's rows depend on rows outside it exactly as in a whole-level launch).
 * n_bands: 0 or the communicator size with a multi-rank communicator.  On one GPU (no communicator, or a one-rank
 * one) the call computes all n_bands bands itself, one launch per band and level -- the rehearsal form used by the
 * tests and by bench.py --banded; d_gathered may then be NULL. */
int sbm_match_batch_device_banded(sbm_ctx* ctx, const void* d_imgs, int64_t frame_stride, int32_t n_frames,
                                  int32_t rows, int32_t cols, int32_t stride, int32_t channels, const void* d_mask,
                                  float threshold, void* d_local, int64_t cap, void* d_gathered,
                                  void* gathered_mirror, int32_t n_bands, void* stream);

/* Detector::match epilogue (line2Dup.cpp:1142-1145) in canonical form: sort by
 * (similarity desc, template_id asc, class_idx asc, y asc, x asc), drop exact
 * duplicates.  Host-side, in place; returns the new count. */
int64_t sbm_canonicalize(sbm_match_rec* recs, int64_t n);

/* ---- match epilogue + NMS on the device ------------------------------------
 * What every reference caller does with Detector::match's list: build Rect(m.x, m.y, templ[0].width, templ[0].height)
 * per match and run cv_dnn::NMSBoxes(boxes, scores, score_threshold, nms_threshold, idx) (include/nms.hpp; test.cpp:491,
 * test_jabil.cpp:148).  For one frame, over the union of its stored records in every part:
 *   1. the epilogue Detector::match applies (line2Dup.cpp:1142-1145), exactly as the facade returns it: sort by
 *      (similarity desc, template_id asc, class_idx asc, y asc, x asc) (sbm_canonicalize's order), then drop a record
 *      equal to its predecessor in (x, y, similarity, class_idx) (Match::operator== under std::unique, which also drops
 *      exact duplicates);
 *   2. NMSBoxes on that list with nms.hpp's arithmetic: keep similarity > score_threshold; if top_k > 0 the first top_k;
 *      greedy walk keeping a box iff its overlap (integer areas, double Jaccard, 1 - (float)distance, 1 when both boxes
 *      are empty) with every kept box is <= the threshold, the threshold multiplied by eta after each kept box while
 *      eta < 1 and it is > 0.5.  A record's box is (x, y, w0, h0), w0 / h0 the level-0 size of the uploaded template
 *      labelled (class_idx, template_id);
 *   3. output: the kept records in walk order (a subsequence of the epilogue list).
 * nms_threshold = 1, score_threshold < 0, top_k = 0 keeps every record (an overlap is at most 1): the call is then the
 * device form of Detector::match's epilogue alone.
 *
 * Layout: n_parts blocks part_stride bytes apart; in block p frame f's records are at d_recs + p * part_stride +
 * f * cap * 24 and its {n_matches, overflow} int32 pair at d_counts + p * part_stride + 8 * f.  Producers:
 *   sbm_match_batch_device: n_parts = 1 (part_stride unused);  sbm_match_device: n_frames = 1 (d_counts: its count, the
 *   overflow word next to it must be zero);  the gathered buffer of sbm_match_{batch_,}device_sharded: d_counts =
 *   d_gathered, d_recs = d_gathered + header, part_stride = one shard, n_parts = world (the sharded merge).
 * Output: frame f's kept records at d_out + f * out_cap (records), {n_kept, flags} at d_out_counts + 2 * f (int32).
 * flags: bit 0 a part overflowed (count > cap or overflow word != 0; the stage ran on the stored records), bit 1
 * n_kept > out_cap (the first out_cap are stored), bit 2 a record that entered the walk carries a label no uploaded
 * template has (its box is empty).
 * Stream-ordered and safe to capture: steady-state calls never synchronise, allocate or read device memory from the
 * host.  The first call after a template upload builds the label -> size table, and a call with a larger
 * n_parts * cap (> 2048 records per frame take global scratch) grows the scratch; both synchronise the device (the rule of
 * sbm_match_batch_device).  Labels that are not unique within the upload: SBM_ERR_INVALID. */
typedef struct sbm_nms_params {
    float score_threshold;
    float nms_threshold;
    float eta;     /* 1 = fixed threshold */
    int32_t top_k; /* 0 = all */
} sbm_nms_params;
int sbm_nms_batch_device(sbm_ctx* ctx, const void* d_recs, const void* d_counts, int64_t cap, int32_t n_frames,
                         int32_t n_parts, int64_t part_stride, const sbm_nms_params* p, void* d_out, int64_t out_cap,
                         void* d_out_counts, void* stream);
/* The host-batch sibling of sbm_match_batch_host_end: enqueues the stage above over the pending batch's device lists and
 * copies back only the kept records: frame f's at out + f * out_cap, {n_kept, flags} at counts + 2 * f.  Ends the batch
 * as _end does.  SBM_ERR_CAPACITY when some frame has flag bit 0 or 1 (its stored records are still returned). */
int sbm_match_batch_host_end_nms(sbm_ctx* ctx, const sbm_nms_params* p, sbm_match_rec* out, int64_t out_cap, int32_t* counts);

/* ---- verify stage on the device: normalised correlation per kept match --------
 * What the reference's production driver does with the matches NMS kept (HCORR, test_jabil.cpp:152-207): cut
 * Rect(match.x, match.y, templ[0].width, templ[0].height) out of the frame, convert it to gray, min-max normalise it to
 * 0..255, correlate it (TM_CCORR_NORMED) with the template's fiducial patch -- the fiducial image scaled and rotated as the
 * template was and cropped to Rect(tl_x, tl_y, width, height) (test_jabil.cpp:187-191 with utils.cpp:157-187) -- and drop
 * the match when the correlation is below 0.8.  Both images have one size, so the correlation map is one number.
 *
 * The arithmetic ("verify rule", csrc/sbm_verify_math.h; DESIGN.md has its standing relative to OpenCV):
 *   1. gray: a 3-channel pixel is B, G, R and becomes (B*1868 + G*9617 + R*4899 + 8192) >> 14; a 1-channel pixel is used
 *      as it is; planar frames give B, G, R from the caller's three planes in the order listed.
 *   2. normalise a gray image with minimum lo and maximum hi: all 0 if hi == lo; else, in double, scale = 255.0 *
 *      (1.0 / (hi - lo)), shift = 0.0 - lo * scale, a = (float)scale, b = (float)shift, and a value g becomes
 *      round-to-nearest-even((float)g * a + b) with both float operations rounded, clamped to 0..255.
 *   3. score: Sab = sum n_roi * n_patch, Saa = sum n_roi^2, Sbb = sum n_patch^2 as unsigned 64-bit integers; den =
 *      sqrt((double)Saa * (double)Sbb); q = den == 0 ? 0 : (double)Sab / den, at most 1; score = (float)q.
 *   4. a record is kept iff (double)score >= min_corr.
 *   5. a record whose label (class_idx, template_id) has no patch, or whose ROI is not wholly inside the frame (or is
 *      empty), is unverifiable: score -1, kept iff keep_unverified != 0.  (The reference would throw.)
 *
 * The patch set: one gray patch per label, of the label's level-0 width x height, rows `stride` bytes apart.  The upload
 * normalises each by rule 2 and stores the normalised bytes and Sbb.  n = 0 clears the set (every record is then
 * unverifiable).  SBM_ERR_INVALID, naming the patch index, for a label the current template upload does not have, a size
 * other than the template's level-0 size, a duplicate label, or stride < width; a refused call leaves the former set in
 * place.  The set belongs to one template upload: after another sbm_upload_templates* call the verify calls return
 * SBM_ERR_STATE until patches are uploaded again.  The upload synchronises the device.
 * sbm_get_verify_patch reads a stored (normalised) patch back, and its Sbb. */
typedef struct sbm_verify_patch {
    int32_t class_idx, template_id, width, height, stride, reserved;
    const uint8_t* gray;
} sbm_verify_patch;
int sbm_upload_verify_patches(sbm_ctx* ctx, const sbm_verify_patch* patches, int32_t n);
int sbm_get_verify_patch(sbm_ctx* ctx, int32_t class_idx, int32_t template_id, uint8_t* out_host, int64_t cap_bytes, uint64_t* sbb);

/* The stage.  The frame arguments are those of sbm_match_batch_device, _ptrs and _planes (the same tables serve).
 * Input: frame f's records at d_recs + f * cap (records), its int32 pair at d_counts + 2 * f -- the output layout of
 * sbm_nms_batch_device, and of sbm_match_batch_device itself ({n_matches, overflow}); min(count, cap) records are read.
 * Output: the kept records at d_out + f * out_cap in input order, their scores (float) at d_scores + f * out_cap,
 * {n_kept, flags} at d_out_counts + 2 * f.  flags: bit 0 the input pair's second word was non-zero or count > cap; bit 1
 * n_kept > out_cap (the first out_cap are stored); bit 2 some record had no patch; bit 3 some ROI was not inside the frame.
 * The output must not overlap the input.  Stream-ordered and safe to capture: steady-state calls never synchronise,
 * allocate or read device memory from the host; a call with a larger n_frames * cap grows the scratch and synchronises the
 * device then.  The scratch is the context's: calls on one context are ordered by their streams.  The output order is the
 * input order on every run. */
typedef struct sbm_verify_params {
    double min_corr;         /* the reference: 0.8 */
    int32_t keep_unverified; /* rule 5 */
    int32_t reserved;
} sbm_verify_params;
int sbm_verify_batch_device(sbm_ctx* ctx, const void* d_imgs, int64_t frame_stride, int32_t n_frames, int32_t rows, int32_t cols,
                            int32_t stride, int32_t channels, const void* d_recs, const void* d_counts, int64_t cap,
                            const sbm_verify_params* p, void* d_out, void* d_scores, int64_t out_cap, void* d_out_counts, void* stream);
int sbm_verify_batch_device_ptrs(sbm_ctx* ctx, const void* d_frame_ptrs, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                                 int32_t channels, const void* d_recs, const void* d_counts, int64_t cap, const sbm_verify_params* p,
                                 void* d_out, void* d_scores, int64_t out_cap, void* d_out_counts, void* stream);
int sbm_verify_batch_device_planes(sbm_ctx* ctx, const void* d_plane_ptrs, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                                   const void* d_recs, const void* d_counts, int64_t cap, const sbm_verify_params* p, void* d_out,
                                   void* d_scores, int64_t out_cap, void* d_out_counts, void* stream);
/* The three stages of the reference's driver (MATCH, NMS, HCORR) for frames in host memory, blocking: uploads the frames
 * into one block of the context's, runs the sbm_match_batch_device path, sbm_nms_batch_device and the verify stage on
 * the context's stream, and copies back only the kept records (frame f's at out + f * out_cap), their scores (scores +
 * f * out_cap) and {n_kept, flags} (counts + 2 * f; the flags of the verify stage, bit 0 where the NMS stage flagged the
 * frame, that is where its raw list overflowed).  cap: records per frame of the raw match lists, and of the NMS stage's
 * output, which therefore never runs out of room.  SBM_ERR_CAPACITY when some frame has flag bit 0 or 1 (the rule of
 * sbm_match_batch_host_end_nms; its stored records are still returned). */
int sbm_match_batch_host_verified(sbm_ctx* ctx, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols,
                                  int32_t stride, int32_t channels, float threshold, int64_t cap, const sbm_nms_params* nms,
                                  const sbm_verify_params* verify, sbm_match_rec* out, float* scores, int64_t out_cap, int32_t* counts);

/* ---- pyramid state ------------------------------------------------------
 * sbm_build_pyramid: the first half of match() (line2Dup.cpp:1084-1120):
 * quantizedOrientations -> [pyrDown -> quantizedOrientations]* -> per level
 * quantize(mask) -> spread -> computeResponseMaps -> linearize, leaving the
 * flat linear memories of every level resident in HBM. */
int sbm_build_pyramid(sbm_ctx* ctx, const uint8_t* img_host, int32_t rows, int32_t cols,
                      int32_t stride, int32_t channels, const uint8_t* mask_host);
/* Install a caller-made one-hot orientation map as level `level` of the
 * pyramid and build its linear memories (spread -> computeResponseMaps ->
 * linearize; line2Dup.cpp:1110-1116).  Levels must be set from 0 upwards. */
int sbm_set_quantized(sbm_ctx* ctx, int32_t level, const uint8_t* quantized_host, int32_t rows,
                      int32_t cols);
/* Read back what a level holds: its one-hot map (rows*cols) and its flat
 * linear memories ([8][lm_stride] bytes; lm_stride >= T*T*W*H, zero tail). */
int sbm_get_quantized(sbm_ctx* ctx, int32_t level, uint8_t* out_host);
/* The one-hot map (ColorGradientPyramid::quantize, line2Dup.cpp:446-450: the orientations under the frame's mask) of
 * frame `frame` of the last batch at `level`; frame 0 is what sbm_get_quantized reads.  SBM_ERR_INVALID for a frame
 * outside the last batch.  A parity-test accessor, like sbm_get_coarse_bitplanes. */
int sbm_get_quantized_frame(sbm_ctx* ctx, int32_t level, int32_t frame, uint8_t* out_host);
int sbm_get_linear_memories(sbm_ctx* ctx, int32_t level, uint8_t* out_host, int64_t cap_bytes,
                            int64_t* lm_stride);
/* The coarsest level's linear memories as BIT planes (round 4): what the coarse pass reads instead of the reference's
 * one byte per (position, orientation) (similarity, line2Dup.cpp:843-856; values {0, 3, 4} of SIMILARITY_LUT :632-635).
 * Per frame 16 planes of lm_stride BITS each, little-endian dwords, in the flat order of the byte linear memories:
 * plane o (0..7): bit j = (LM[o][j] > 0); plane 8 + o: bit j = (LM[o][j] == 4).  frame: which frame of the last batch.
 * out_host: 16 * lm_stride / 8 bytes.  Fails with SBM_ERR_STATE when the last call did not produce them (a threshold < 0,
 * or sbm_set_coarse_mode picked a byte kernel).  A parity-test accessor. */
int sbm_get_coarse_bitplanes(sbm_ctx* ctx, int32_t frame, uint8_t* out_host, int64_t cap_bytes);
/* Which kernel form the last coarse pass of this context ran (every form is timed as "k_similarity_coarse"):
 * out = {kind, P, wide, dw}.  kind: 0 none launched yet, 1 the byte kernel with four waves per item, 2 the byte kernel
 * with one wave per item, 3 the bit-plane kernel with one wave per item, 4 the bit-plane kernel with eight waves per
 * item.  P: counter planes (7, 10 or 13; kinds 3 and 4), wide: 1 for the wide batch schedule, dw: dwords per lane (1 or
 * 2; kind 3); 0 where they do not apply.  A call replayed from a captured graph reports the form it was captured with.
 * Reads a host-side record: no device work, no synchronisation, no state change.  A parity-test accessor. */
int sbm_get_coarse_form(sbm_ctx* ctx, int32_t out[4]);
/* Which kernel form the last refinement pass of this context ran at `level` (a level below the coarsest; every form is timed
 * as "k_similarity_local"): out = {kind, LW, order, t8, sparse, slots}.  kind: 0 nothing launched for this level yet, 1 the
 * byte kernel on the 8 response planes, 2 on the plane of spread bytes row-major, 3 on the same plane in strips, 4 the
 * bit-strip kernel.  LW: waves per candidate (1 for kind 4, else 4 or 16), order: 0 per-frame slots or 2 the frame-major list,
 * t8: 1 for the strip kernel's T = 8 instantiation, sparse: 1 where level 0's bit strips were built for this call's
 * candidates only, slots: candidate slots per frame of the grid.  A call replayed from a captured graph reports the form it
 * was captured with.  SBM_ERR_INVALID for the coarsest level or a level outside the pyramid.  Reads a host-side record: no
 * device work, no synchronisation, no state change.  A parity-test accessor. */
int sbm_get_refine_form(sbm_ctx* ctx, int32_t level, int32_t out[6]);
/* Which form of the source pass the last call of this context launched (both are timed as "k_quantize"): 0 none -- the call
 * built level 0's map whole, or no call yet --, 1 the strided form of the streaming gradient kernel, 2 the line-shaped kernel
 * that takes layouts whose first pixel, row stride and frame stride are multiples of 4 bytes, whose frame fits 32-bit offsets
 * and whose width is a multiple of 64 (SBM_SOURCE_LINES=0 in the environment: never).  A call replayed from a captured graph
 * reports the form it was captured with.  Reads a host-side record, like sbm_get_coarse_form.  A parity-test accessor. */
int sbm_get_source_form(sbm_ctx* ctx, int32_t* out);
/* out = {calls whose source pass stored the retained copy of level 0's source, calls whose source pass left it unwritten}, over
 * the life of the context.  A call of the sparse level-0 path on frames a fixed number of bytes apart stores the copy only while
 * no later match call is enqueued on the context behind it: the copy's readers -- sbm_get_quantized*, sbm_set_quantized(0),
 * the stage entry points and the template loop on the resident pyramid -- see the last call's state, and wait for that call.
 * The call's frames must stay valid until its work is done.  Calls on a table of frame or plane pointers, and every call with
 * SBM_RETAIN_ALWAYS=1 in the environment, always store it; a call that builds level 0's map whole counts in neither.  The
 * totals are device counters: the getter waits for the device.  A parity-test accessor. */
int sbm_get_source_retention(sbm_ctx* ctx, int32_t out[2]);
/* The sparse level-0 gradient launch of the last call of this context: out = {selection, working, launched}.  selection: 0 the
 * call made no such launch (level 0's map was built whole, or no call yet), 1 its work items were chosen by the refinement-tile
 * flags on the fixed strip grid, 2 by the record of need rectangles (per band of 8 pixel rows the hull of the map columns some
 * coarse candidate's refinement depends on; SBM_SPARSE_RECTS=0 in the environment: never).  working: the work items that did
 * not return at once, counted on the device only while profiling is enabled (sbm_set_profiling), -1 otherwise and for a call
 * replayed from a captured graph; with sbm_match's overflow retry, the retry's launch.  launched: the work items of the grid.
 * Waits for the device when a count is still outstanding.  A parity-test accessor. */
int sbm_get_sparse_items(sbm_ctx* ctx, int32_t out[3]);
/* {list_mode, slots_per_frame, list_rows} of the last call's sparse level-0 gradient launch: list_mode 1 when it ran, by
 * slots_per_frame waves per frame, from the per-frame lists of working items that the mark launch leaves (0, 0, 0: a wave per
 * item, each testing itself, or no sparse launch at all).  list_rows: the rows per work item of the grid the lists are made on,
 * which a listed frame's items have; a frame without a list, the packed last-strip waves and the number of waves launched keep
 * the launch's own rows per item (SBM_SPARSE_LIST_HS=0 in the environment: the lists are made on that grid too). */
int sbm_get_sparse_list(sbm_ctx* ctx, int32_t out[3]);
/* How the linear memories of `level` were last built: out = {current, form, builder, split, allty, packed}.  current: the
 * buffers that hold the level's current contents, as a bit set: 1 the 8 response planes, 2 the plane of spread bytes, 4 that
 * plane is strip-interleaved, 8 the bit strips, 16 the coarsest level's bit planes.  form: the form of the last build, -1 none
 * yet, 0 the 8 response planes, 1 the spread plane row-major, 2 the same in strips, 3 bit planes, 4 bit strips, 5 bit strips in
 * the tiles the call's coarse candidates read only.  builder: 0 none, 1 the one-launch builder for strides 4 and 8, 2 the batched
 * any-stride builder, 3 the generic single-frame builder, 4 the unfused spread / response / linearize kernels.  split, allty:
 * work items per (pixel row, 4 cells) of an 8-plane level, and 1 where a thread built all four sub-rows of its cells (builder 1;
 * else 0).  packed: 1 the bit planes were since packed from the spread plane, 2 from the 8 response planes, 0 neither.  A call
 * replayed from a captured graph reports what it was captured with.  Reads a host-side record: no device work, no
 * synchronisation, no state change.  A parity-test accessor. */
int sbm_get_level_build(sbm_ctx* ctx, int32_t level, int32_t out[6]);
/* One frame's whole share of one buffer of `level`, zero tail included, exactly as it lies in device memory.  which: 0 the 8
 * response planes (8 * lm_stride bytes), 1 the plane of spread bytes (lm_stride), 2 the bit strips (the strips' dwords, then a
 * zero tail up to the frame stride), 3 the refinement-tile flags of level 0 (one byte per tile).  *bytes: the size of that share;
 * out_host may be null to ask for it alone.  Waits for the device and copies: nothing is rebuilt, expanded or completed, and the
 * record of current buffers does not change -- whether the buffer is current is sbm_get_level_build's to say.  SBM_ERR_STATE
 * when the buffer is not allocated, SBM_ERR_INVALID for a frame outside the last batch.  A parity-test accessor. */
int sbm_get_level_stored(sbm_ctx* ctx, int32_t level, int32_t frame, int32_t which, uint8_t* out_host, int64_t cap_bytes,
                         int64_t* bytes);
int sbm_level_dims(sbm_ctx* ctx, int32_t level, int32_t* rows, int32_t* cols);

/* Second half of match(): Detector::matchClass over the selected templates
 * (line2Dup.cpp:1160-1297) against the resident pyramid. */
int sbm_match_templates(sbm_ctx* ctx, float threshold, sbm_match_rec* out_host, int64_t cap,
                        int64_t* n_out);

/* Asynchronous form: the template loop against the resident pyramid on `stream`, results into
 * caller-provided device buffers (as sbm_match_device). */
int sbm_match_templates_device(sbm_ctx* ctx, float threshold, void* d_out, int64_t cap, void* d_count,
                               void* stream);

/* ---- single reference functions (stage entry points; host arrays) --------
 * Each runs the HIP kernel that replaces one reference function and copies the
 * result back, so it can be tested (and adopted) on its own. */

/* quantizedOrientations + hysteresisGradient (line2Dup.cpp:313-404, 218-311).
 * magnitude / angle_ori (float, rows*cols) may be NULL; angle is the one-hot map. */
int sbm_quantized_orientations(sbm_ctx* ctx, const uint8_t* img_host, int32_t rows, int32_t cols,
                               int32_t stride, int32_t channels, float weak_threshold,
                               float* magnitude, uint8_t* angle, float* angle_ori);
/* The per-pixel scan of ColorGradientPyramid::extractTemplate (line2Dup.cpp:452-539; training side): the pixels of
 * [2, rows-2) x [2, cols-2) that pass the 3x3-eroded mask (NULL: all), whose squared magnitude exceeds
 * strong_threshold^2 and that the reference's row-major `magnitude_valid` scan accepts as 5x5 local maxima -- found
 * by a data-parallel kernel (no strictly larger neighbour), ties among equal neighbours resolved in row-major order on
 * the host exactly as the sequential scan does.  xy[i] = x | y << 16, in row-major order; *n_out = their number
 * (SBM_ERR_CAPACITY if > cap).  The orientation test (:504) and the feature selection stay with the caller. */
int sbm_extract_local_maxima(sbm_ctx* ctx, const float* magnitude_host, const uint8_t* mask_host, int32_t rows, int32_t cols,
                             float strong_threshold, int32_t* xy, int64_t cap, int64_t* n_out);
/* The 16-bin quantisation of hysteresisGradient (line2Dup.cpp:225: convertTo(CV_8U, 16/360) of the
 * phase image) as the match path computes it: an integer rule on the Sobel gradient (gx, gy), exact for
 * |gx|, |gy| <= 1020.  q16[i] in 0..16. */
int sbm_orientation_bins(sbm_ctx* ctx, const int16_t* gx, const int16_t* gy, int64_t n, uint8_t* q16);
/* cv::resize(src, dst, cv::Size(), fx, fy) (INTER_LINEAR, 8-bit) as shapeInfo_producer::transform calls it to make
 * the scaled training images (line2Dup.h:379-405).  Output size = (cvRound(rows*fy), cvRound(cols*fx)), written to
 * out_rows / out_cols; out == NULL only queries the size. */
int sbm_resize_linear(sbm_ctx* ctx, const uint8_t* img_host, int32_t rows, int32_t cols, int32_t stride, int32_t channels,
                      double fx, double fy, uint8_t* out, int64_t cap_bytes, int32_t* out_rows, int32_t* out_cols);
/* cv::pyrDown as called by ColorGradientPyramid::pyrDown (line2Dup.cpp:431-433). */
int sbm_pyrdown(sbm_ctx* ctx, const uint8_t* img_host, int32_t rows, int32_t cols, int32_t stride,
                int32_t channels, uint8_t* out_host);
/* spread (line2Dup.cpp:616-630). */
int sbm_spread(sbm_ctx* ctx, const uint8_t* src_host, int32_t rows, int32_t cols, int32_t T,
               uint8_t* dst_host);
/* computeResponseMaps (line2Dup.cpp:637-747): maps_host is [8][rows*cols]. */
int sbm_compute_response_maps(sbm_ctx* ctx, const uint8_t* spread_host, int32_t rows, int32_t cols,
                              uint8_t* maps_host);
/* linearize (line2Dup.cpp:749-777): lm_host is [T*T][(rows/T)*(cols/T)]. */
int sbm_linearize(sbm_ctx* ctx, const uint8_t* map_host, int32_t rows, int32_t cols, int32_t T,
                  uint8_t* lm_host);
/* similarity / similarity_64 (line2Dup.cpp:807-858, 924-984) of uploaded
 * template `template_index` at the coarsest level of the resident pyramid:
 * dst_host is the H x W uint16 score map. */
int sbm_similarity(sbm_ctx* ctx, int32_t template_index, uint16_t* dst_host);
/* similarityLocal / similarityLocal_64 (line2Dup.cpp:860-922, 986-1048) at
 * pyramid level `level` around centre (cx, cy): dst_host is 16 x 16 uint16. */
int sbm_similarity_local(sbm_ctx* ctx, int32_t level, int32_t template_index, int32_t cx,
                         int32_t cy, uint16_t* dst_host);

/* ---- batched template training ---------------------------------------------
 * Detector::addTemplate (line2Dup.cpp:1299-1353) for n_images images of one geometry, on the device from the gradient
 * stage to cropTemplates: per pyramid level (n_levels and weak_threshold are the context's) quantised orientations,
 * pyrDown and the nearest-neighbour mask of the next level, then the 5x5 local maxima above strong_threshold under the
 * 3x3-eroded mask, their ties resolved in row-major order as extractTemplate's scan does (:452-539), the candidates in
 * std::stable_sort's order, selectScatteredFeatures (:163-212; num_features halves per level, :427) and cropTemplates
 * (:115-161) -- every kernel after the gradients launched once for the batch.  Image i is exactly what addTemplate
 * makes of it alone:
 *   levels[i * n_levels + l]   the template of level l; feature_offset counts from the image's feature block, level l's
 *                              features directly behind level l-1's
 *   feats[i * feat_cap ...]    the image's features (theta = Feature::theta, the unquantised angle)
 *   status[2 * i]              0 ok | 1 too few candidates at some level (where addTemplate returns -1) | 2 feat_cap too
 *                              small; nothing else of an image that is not ok is valid
 *   status[2 * i + 1]          the image's number of features (status 0 and 2), the failing level (status 1)
 * One image's failure does not touch another image's output.  rows, cols <= 32767. */
typedef struct sbm_train_feature {
    int32_t x, y, label;
    float theta;
} sbm_train_feature;

/* Device form: image i at d_imgs + i * img_stride bytes (rows of `stride` bytes).  d_masks: NULL = no mask;
 * mask_stride == 0 = one mask for all images; any other stride must be >= rows * cols (SBM_ERR_INVALID otherwise).
 * d_levels: n_images * n_levels sbm_template_level; d_feats: n_images * feat_cap sbm_train_feature; d_status:
 * n_images * 2 int32.  Stream-ordered on `stream` (NULL: the context's); the scratch grows on a first call of a larger
 * batch or geometry (which waits for the device, as sbm_match_batch_device does); steady-state calls do not synchronise.
 * A context has ONE training scratch: calls on one context must be ordered by the caller (the same stream, or events
 * between streams) -- two calls in flight on different streams would share it.  Use a context per stream to overlap. */
int sbm_train_batch_device(sbm_ctx* ctx, const void* d_imgs, int64_t img_stride, int32_t n_images, int32_t rows,
                           int32_t cols, int32_t stride, int32_t channels, const void* d_masks, int64_t mask_stride,
                           float strong_threshold, int32_t num_features, void* d_levels, void* d_feats,
                           int64_t feat_cap, void* d_status, void* stream);
/* Host form: imgs[i] (rows of `stride` bytes); masks may be NULL, and so may any masks[i] (no mask for that image).
 * Uploads, runs the device form on the context's stream, downloads and synchronises. */
int sbm_train_batch(sbm_ctx* ctx, const uint8_t* const* imgs, int32_t n_images, int32_t rows, int32_t cols,
                    int32_t stride, int32_t channels, const uint8_t* const* masks, float strong_threshold,
                    int32_t num_features, sbm_template_level* levels, sbm_train_feature* feats, int64_t feat_cap,
                    int32_t* status);

/* ---- ragged batched training -------------------------------------------------
 * The same, for images of different sizes and feature counts in one call: the training loop of the reference's
 * test.cpp:scale_test("train") (:162-200) calls addTemplate on shapes.src_of(info) over scale_range {0.1, 1} in steps of
 * 0.01, 91 sources of 91 sizes, which as one-geometry batches are 91 batches of one image.  Here every kernel after the
 * per-image gradient launches runs once for the batch, the image (and the pyramid level) a grid dimension; each
 * (image, level) reads its own record of a device table, so a batch costs about its largest image, not the sum.
 * Image i is exactly what sbm_train_batch makes of it alone; one image's failure or overflow touches nothing of another.
 *   levels[i * n_levels + l], status[2 * i], status[2 * i + 1]   as sbm_train_batch
 *   feats[images[i].feat_first ...]   the image's block of images[i].feat_cap records; feature_offset counts from it
 * An image too small for the pyramid is no error of the call: levels are built while both sides are >= 5 (the 5 x 5
 * scan of extractTemplate, :452-539, has no pixel in a smaller one), and the image ends with status {1, first failing
 * level} as addTemplate returns -1 for it (:1343) and the loop goes on.  SBM_ERR_INVALID, with nothing enqueued:
 * n_images outside 1 .. 65535, channels not 1 or 3, rows or cols outside 1 .. 32767, stride < cols * channels,
 * num_features < 1 or halved to fewer than 2 at the last level, a negative feat_cap or feat_first, feature blocks that
 * overlap, a null image.  Fewer than 2, not 1 as in sbm_train_batch: asked for ONE feature, selectScatteredFeatures
 * (:163-212) never returns once the level has a candidate (its first candidate is always enough, so it clears and
 * widens the distance for ever), and a kernel that follows it would not end; these calls refuse the count instead. */
typedef struct sbm_train_image { /* 48 bytes */
    const void* img;             /* first pixel; a device address in the _device form, a host address in the host form */
    const void* mask;            /* rows x cols bytes, rows packed; NULL: none */
    int32_t rows, cols, stride, num_features;
    int64_t feat_first, feat_cap; /* this image's block of the feature array, in records */
} sbm_train_image;

/* Device form.  `images` is a HOST array, read during the call only; img and mask are device addresses.  d_levels:
 * n_images * n_levels sbm_template_level; d_feats: the feature array the blocks lie in; d_status: n_images * 2 int32.
 * Stream-ordered on `stream` (NULL: the context's): the table of records travels on the stream from a pinned slot, so
 * calls enqueued back to back need no synchronisation between them -- a call waits on the host only for the PREVIOUS
 * call's table copy to have left the slot, and for the device when the scratch has to grow.  The
 * one-training-scratch-per-context rule of sbm_train_batch_device stands.  Not capturable into a hipGraph (the host
 * wait, and the table's contents are the call's). */
int sbm_train_ragged_device(sbm_ctx* ctx, const sbm_train_image* images, int32_t n_images, int32_t channels,
                            float strong_threshold, void* d_levels, void* d_feats, void* d_status, void* stream);
/* Host form: img and mask are host addresses, feats a host array that holds every block.  Uploads, runs the device form
 * on the context's stream, downloads and synchronises. */
int sbm_train_ragged(sbm_ctx* ctx, const sbm_train_image* images, int32_t n_images, int32_t channels,
                     float strong_threshold, sbm_template_level* levels, sbm_train_feature* feats, int32_t* status);

/* The scale sweep of shapeInfo_producer (line2Dup.h:379-405, 451-457: transform resizes the source, mask_of the mask and
 * thresholds it `> 0`): scale k trains cv::resize(img, Size(), fx, fy) under the equally resized mask, non-zero staying
 * non-zero.  One source, uploaded once; one resize launch for all scales (sizes as sbm_resize_linear(out = NULL)
 * reports them); the scaled images live in the context's scratch, and from there on the call is the ragged one, scale k
 * its image k.  A scale that resizes to an empty image: SBM_ERR_INVALID for the call.  Not capturable either. */
typedef struct sbm_train_scale {
    double fx, fy;
    int32_t num_features, reserved;
    int64_t feat_first, feat_cap;
} sbm_train_scale;

int sbm_train_sweep_device(sbm_ctx* ctx, const void* d_img, int32_t rows, int32_t cols, int32_t stride, int32_t channels,
                           const void* d_mask, const sbm_train_scale* scales, int32_t n_scales, float strong_threshold,
                           void* d_levels, void* d_feats, void* d_status, void* stream);
int sbm_train_sweep(sbm_ctx* ctx, const uint8_t* img_host, int32_t rows, int32_t cols, int32_t stride, int32_t channels,
                    const uint8_t* mask_host, const sbm_train_scale* scales, int32_t n_scales, float strong_threshold,
                    sbm_template_level* levels, sbm_train_feature* feats, int32_t* status);

/* ---- rotated template families -------------------------------------------------
 * Detector::addTemplate_rotate (line2Dup.cpp:1395-1451) for n_bases trained pyramids and n_thetas angles each, in one
 * call on the device: the reference's demo trains one template and calls addTemplate_rotate once per angle
 * (test.cpp:303-313).  Pair p = b * n_thetas + k is exactly what addTemplate_rotate(class, base b, thetas[k],
 * centre of b) makes of that pair alone -- every rounding step of the rotation kept (float differences, double
 * products and sums without fused multiply-add, truncation of r + 0.5f), the orientation wrapped and its label taken
 * as there, cropTemplates (:115-161) over the pair's levels.  cos and sin of each angle are computed once on the host
 * and travel to the kernel as a table, so no device libm enters the result.
 *   levels[p * n_levels + l]   the rotated template of level l; feature_offset counts from the pair's feature block,
 *                              level l's features directly behind level l-1's
 *   feats[bases[b].out_first + k * bases[b].out_cap ...]   the pair's block of out_cap records
 *   status[2 * p], status[2 * p + 1]
 *       {0, features}          ok
 *       {1, level}             the base's own training failure: its status pair began with 1, and the pair is copied
 *       {2, features needed}   out_cap too small
 *       {3, reason}            the base is not rotatable: 1 its status pair is neither ok nor a training failure (its
 *                              features overflowed their block), 2 it has no feature at all or a level's n_features
 *                              is outside 0 .. 8191, 3 a feature lies outside the domain below
 * The level records of a pair that is not ok are zeroed, as in training; one pair never touches another's output.
 * Domain: every theta finite with |theta| <= 36000, every centre component finite with |c| <= 65536 (SBM_ERR_INVALID
 * otherwise, nothing enqueued); every base feature's theta finite and in [-720, 720] and its coordinate (x + tl_x,
 * y + tl_y) in 0 .. 32767 -- in the device form the host cannot see these, so a feature outside gives its pairs status
 * {3, 3}; the wrap loops of the orientation carry a fixed bound (103 steps) and cannot spin.
 * SBM_ERR_INVALID, with nothing enqueued: a null argument, n_bases or n_thetas < 1, n_bases * n_thetas >
 * 2^31 / n_levels, a negative out_first or out_cap, output blocks (a base's n_thetas * out_cap records from out_first)
 * that overlap, a theta or a centre outside the domain.  Output blocks must not overlap any base's own features. */
typedef struct sbm_rotate_base {          /* one trained pyramid and where its rotations go (48 bytes) */
    const sbm_template_level* levels;     /* n_levels records, as sbm_train_* wrote them (tl_x/tl_y set) */
    const sbm_train_feature*  feats;      /* the block the levels' feature_offset counts from */
    const int32_t*            status;     /* NULL, or the base's status pair from a training call */
    float center_x, center_y;             /* level-0 centre of rotation */
    int64_t out_first, out_cap;           /* rotation k's feature block: [out_first + k*out_cap, +out_cap) */
} sbm_rotate_base;

/* Device form.  `bases` and `thetas` are HOST arrays, read during the call only; the pointers inside a record are
 * device addresses, and may be the very output buffers of a preceding sbm_train_*_device call on the same stream
 * (sweep, then rotate, never returning to the host).  d_levels: n_bases * n_thetas * n_levels sbm_template_level;
 * d_feats: the feature array the blocks lie in; d_status: n_bases * n_thetas * 2 int32.  Stream-ordered on `stream`
 * (NULL: the context's): the records and the angle table travel on the stream from the pinned slot of the ragged
 * training table, so calls enqueued back to back need no synchronisation between them.  The
 * one-training-scratch-per-context rule of sbm_train_batch_device stands.  Not capturable into a hipGraph (the host
 * wait for the slot, and the tables' contents are the call's). */
int sbm_train_rotate_device(sbm_ctx* ctx, const sbm_rotate_base* bases, int32_t n_bases, const float* thetas,
                            int32_t n_thetas, void* d_levels, void* d_feats, void* d_status, void* stream);
/* Host form: levels, feats and status inside the records are host addresses (a base's features are read up to the end
 * its level records give), and so are levels, feats and status of the result.  Uploads, runs the device form on the
 * context's stream, downloads and synchronises; of the feature array only the blocks of pairs that are ok are written. */
int sbm_train_rotate(sbm_ctx* ctx, const sbm_rotate_base* bases, int32_t n_bases, const float* thetas,
                     int32_t n_thetas, sbm_template_level* levels, sbm_train_feature* feats, int32_t* status);

/* ---- device-trained families as the match set ---------------------------------------
 * sbm_upload_templates for pyramids that lie in device memory as a sbm_train_*_device call wrote them: the loop of
 * addTemplate / addTemplate_rotate that fills the reference's TemplatesMap (test.cpp:303-313; line2Dup.cpp:1299-1353,
 * :1395-1451) ends in the map matchClass walks (:1160-1172), and here in the context's template set, without the
 * features leaving the device.  A source is a run of n_pyramids pyramids of one class: pyramid i's n_levels level
 * records at d_levels + i * n_levels, its feature block the records [feat_first + i * feat_pitch, + feat_cap) of
 * d_feats (a level's feature_offset counts from the block's start and its features must lie inside the block), its
 * status pair at d_status + 2 * i (NULL: every pyramid is ok).
 *   sbm_train_batch_device:   feat_first = 0, feat_pitch = feat_cap
 *   sbm_train_rotate_device:  one source per base, feat_first = out_first, feat_pitch = feat_cap = out_cap
 *   ragged images / a sweep's scales with irregular feat_first: one source each
 * The reference demo's family is two sources of one class: the base, then its rotations.
 * Kept: a pyramid whose status pair begins with 0.  Any other pyramid is skipped, which is no error: addTemplate returns
 * -1 for it and adds nothing (line2Dup.cpp:1343).  The kept pyramids become templates 0, 1, ... in source order;
 * template_id is the running count of kept pyramids of the pyramid's class_idx (line2Dup.cpp:1312);
 * template_index_out[j] (host, may be NULL) is the template index of input pyramid j over all sources, -1 if skipped.
 * Afterwards the context holds exactly what sbm_upload_templates leaves for the kept pyramids' level records, their
 * features without theta and those class and id arrays -- every device table byte for byte, features packed tightly in
 * template and level order -- and the same state changes apply (every class selected, graphs dropped).  Zero kept
 * pyramids give an empty set.
 * `sources` is a host array, read during the call only.  The kernels run on `stream` (NULL: the context's), behind the
 * training calls that made the sources: no synchronisation is needed between training and this call.  The call waits
 * for the device before it swaps the tables, as sbm_upload_templates does; it is not capturable.  Only the kept
 * pyramids' level sizes, the kept flags and a verdict reach the host, never a feature.
 * SBM_ERR_INVALID, the former template set untouched and still matchable, the message naming source, pyramid and level:
 * a null argument; n_sources < 1; a negative n_pyramids, feat_first, feat_pitch or feat_cap; more than 2^31 / n_levels
 * pyramids; a kept pyramid with a level whose n_features is outside 0 .. 8191 (CV_Error, line2Dup.cpp:1195, :1260) or
 * whose [feature_offset, + n_features) leaves [0, feat_cap) -- the first such level in source order; otherwise 2^31 - 1
 * features or more in total; otherwise a feature with x or y outside 0 .. 65535 or a label outside 0 .. 7 (CV_DbgAssert,
 * line2Dup.cpp:788-789), the first in source order. */
typedef struct sbm_template_source {  /* a run of trained pyramids in device memory (56 bytes) */
    const void* d_levels;   /* n_pyramids * n_levels sbm_template_level, as a sbm_train_* call wrote them */
    const void* d_feats;    /* the sbm_train_feature array the pyramids' blocks lie in */
    const void* d_status;   /* n_pyramids status pairs of that call, or NULL: every pyramid is ok */
    int32_t n_pyramids;
    int32_t class_idx;      /* label of every pyramid of the run */
    int64_t feat_first, feat_pitch, feat_cap; /* pyramid i's block: records [feat_first + i*feat_pitch, +feat_cap) */
} sbm_template_source;

int sbm_upload_templates_device(sbm_ctx* ctx, const sbm_template_source* sources, int32_t n_sources,
                                int32_t* template_index_out, void* stream);

/* The installed set in the input form of sbm_upload_templates, after either upload: levels_out [n_templates][n_levels]
 * (width, height, n_features and a tightly packed feature_offset as the context holds them; tl_x = tl_y = 0, which the
 * match path never reads; pyramid_level = the level), feats_out up to feat_cap records, class_idx_out and
 * template_id_out n_templates each.  Any output may be NULL; n_templates / n_features are always written, so a call with
 * NULL outputs queries the sizes.  SBM_ERR_CAPACITY when feats_out is given and feat_cap < n_features.  Waits for the
 * device and copies; changes no state.  A parity-test accessor. */
int sbm_get_templates(sbm_ctx* ctx, sbm_template_level* levels_out, sbm_feature* feats_out, int64_t feat_cap,
                      int32_t* class_idx_out, int32_t* template_id_out, int32_t* n_templates, int64_t* n_features);
/* One template table exactly as it lies in device memory.  which: 0 the level records {width, height, n_features,
 * feature_offset} int32 per (template, level); 1 the features x | y << 16; 2 their labels (bytes); 3 their levels (bytes);
 * 4 and 5 the copies of 1 and 2 sorted inside each (template, level) by (x / T) & 15 (stable); 6 the 17 uint16 class
 * offsets of those per (template, level); 7 largest x | largest y << 16 per (template, level); 8 class_idx and 9
 * template_id per template.  *bytes: the table's size; out_host may be NULL to ask for it alone.  Waits for the device
 * and copies; changes no state.  SBM_ERR_CAPACITY when cap_bytes is too small.  A parity-test accessor. */
int sbm_get_template_table(sbm_ctx* ctx, int32_t which, void* out_host, int64_t cap_bytes, int64_t* bytes);

/* ---- measurement ---------------------------------------------------------
 * Per-kernel HIP-event timings of the last sbm_match/sbm_build_pyramid/
 * sbm_match_templates call when profiling was enabled (adds synchronisation;
 * never enabled in the throughput path). names/ms arrays hold up to cap entries.
 * enabled = 2: the timings of successive asynchronous calls accumulate (no per-call reset) until
 * sbm_get_timings has returned all of them -- the way to time kernels while several streams are in flight. */
int sbm_set_profiling(sbm_ctx* ctx, int32_t enabled);
int sbm_get_timings(sbm_ctx* ctx, const char** names, float* ms, int32_t cap, int32_t* n);
/* Algorithmic bytes of the coarse pass for the selected templates on the
 * resident pyramid: sum over in-bounds coarsest-level features of
 * max(template_positions, 0)  (SURVEY.md 8d). */
int sbm_coarse_bytes(sbm_ctx* ctx, int64_t* bytes);

/* Counters of the last template-matching call: coarse candidates found
 * (line2Dup.cpp:1208-1214) and the bytes the refinement passes read for frame 0,
 * sum over refined candidates of nf_level * 256 on response / spread bytes (the
 * reference's figure) and nf_level * 128 on bit strips
 * (sbm_set_refine_bits); accumulated only while profiling is enabled, to keep the
 * atomic out of the throughput path.  Synchronises. */
int sbm_get_stats(sbm_ctx* ctx, int64_t* n_candidates, int64_t* refine_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SBM_H */
