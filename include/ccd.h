/*
 * ccd.h - C ABI of the MI355X-native Cool-chic decoder (libccd.so).
 *
 * Drop-in boundary for the reference's decode path (paths relative to /root/reference):
 *   cc_decode.py:14-20                                  -> ccd_decode_video()
 *   coolchic/bitstream/decode.py:26   decode_video()    -> ccd_decode_video()
 *   coolchic/bitstream/decode.py:96   decode_frame()    -> ccd_batch_* (one frame = 1-2 cool-chics)
 *   coolchic/bitstream/component/coolchic.py:29
 *        encode_decode_coolchic(mode="decode")          -> ccd_decode_coolchic(), ccd_batch_*
 *   coolchic/bitstream/header/header.py:72 read_header  -> ccd_read_*_header()
 *
 * Conventions: plain pointers and sizes, no torch types; status-code
 * returns (0 = ok, <0 = error, see ccd_strerror); caller-owned output buffers; one HIP stream
 * per call; process-wide state is limited to per-device caches and helper streams (see the note at ccd_pool_trim); inputs are
 * never modified.  Device pointers are ordinary
 * hipMalloc'ed addresses (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as
 * void* (e.g. torch.cuda.current_stream().cuda_stream), NULL = the default stream.
 *
 * The library has NO CPU fallback: every compute entry point fails with CCD_ERR_HIP when no
 * gfx950 device is usable.
 */
#ifndef CCD_H
#define CCD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCD_MAX_GRIDS 40
#define CCD_MAX_SYN_LAYERS 8
#define CCD_MAX_REFS 2

enum {
    CCD_OK = 0,
    CCD_ERR_TRUNCATED = -1,    /* bitstream shorter than its headers claim */
    CCD_ERR_VALUE = -2,        /* header field out of range (reference: ValueError, element.py:289-292) */
    CCD_ERR_INVALID_DATA = -3, /* range decoder met an impossible quantile (constriction: InvalidData) */
    CCD_ERR_UNSUPPORTED = -4,  /* legal stream using a feature this build does not implement yet */
    CCD_ERR_NOMEM = -5,
    CCD_ERR_HIP = -6,          /* HIP runtime error / no usable device */
    CCD_ERR_ARG = -7           /* bad argument (reference: ValueError, coolchic.py:39-51) */
};

const char* ccd_strerror(int code);
/* "ccd <version> gfx950" */
const char* ccd_version(void);

/* ---- headers (host only; reference: bitstream/header/header.py) ------------------------- */
typedef struct {
    int32_t n_frames, n_intras, n_p_frames, n_bytes_header;
    int32_t intra_pos[4096];
    int32_t p_pos[4096];
} ccd_video_header; /* header.py:130-147 */

typedef struct {
    int32_t display_index;
    int32_t frame_type;      /* 0 I, 1 P, 2 B */
    int32_t frame_data_type; /* 0 rgb, 1 yuv420, 2 yuv444, 3 flow */
    int32_t bitdepth;        /* 8..16 */
    int32_t n_bytes_header;
    int32_t n_refs;
    int32_t index_references[CCD_MAX_REFS];
    int32_t global_flow[2 * CCD_MAX_REFS];
    int32_t warp_filter_size;
} ccd_frame_header; /* header.py:172-218 */

typedef struct { int32_t out_ft, k_size, mode /*0 linear 1 residual*/, non_linearity /*0 none 1 relu*/; } ccd_syn_layer;

typedef struct {
    /* transmitted fields, header.py:244-325 */
    int32_t linear_stabiliser_synth, n_layer_synthesis, ups_k_size, ups_preconcat_k_size;
    int32_t output_feature_ifce, spatial_context_arm, linear_stabiliser_arm, n_hidden_layers_arm;
    int32_t img_size[2];
    int32_t latent_resolution[2];
    int32_t n_latent_grids;
    int32_t flag_hyperlatent, flag_common_randomness;
    int32_t final_upsampling_type; /* 0 nearest 1 bilinear 2 bicubic */
    int32_t nn_q_step_log2[8];     /* arm.w arm.b ifce.w ifce.b ups.w ups.b syn.w syn.b */
    int32_t nn_expgol_cnt[8];
    int32_t nn_n_bytes, nn_n_bit_pad, n_bytes_latent, n_bytes_header;
    int32_t has_ifce_resolution;
    int32_t ifce_resolution[2];
    int32_t hyperlatent_resolution[2];
    ccd_syn_layer syn_layer[CCD_MAX_SYN_LAYERS];
    /* derived geometry, component/core/coolchic.py:149-225 */
    int32_t n_grids;
    int32_t grid_h[CCD_MAX_GRIDS], grid_w[CCD_MAX_GRIDS];
    int32_t is_hyperlatent[CCD_MAX_GRIDS];
    int32_t input_features_ifce[CCD_MAX_GRIDS];
    int32_t input_feature_synthesis;
    int32_t total_context_arm;
    int32_t out_channels; /* synthesis output channels */
    int64_t n_symbols;    /* total latent symbols */
} ccd_cc_header;

/* Each returns the number of header bytes consumed (> 0) or an error (< 0). */
int ccd_read_video_header(const uint8_t* p, size_t n, ccd_video_header* h);
int ccd_read_frame_header(const uint8_t* p, size_t n, ccd_frame_header* h);
int ccd_read_cc_header(const uint8_t* p, size_t n, ccd_cc_header* h);

/* VideoHeader.get_coding_structure() (header.py:161 -> utils/codingstructure.py:226-436 CodingStructure.compute_coding_struct):
 * the frames a video header implies, in CODING order.  Each array receives h->n_frames entries (refs: 2 per frame, display
 * orders, -1 where unused; frame_type 0 I / 1 P / 2 B; depth as the reference counts it).  Returns n_frames, or
 * CCD_ERR_VALUE where the reference asserts (first frame not intra, last frame neither intra nor P, a frame both I and P).
 * Positions listed twice are CCD_ERR_VALUE too: the reference only prints a warning, builds a structure that lacks a display
 * index and fails after decoding (decode.py:86 on None).  ccd_decode_video decodes in this order with these references, like
 * decode.py:67-75 (the frame headers' display_index / index_references are not read there).  The frame header's frame_type
 * decides the number of cool-chics and the reconstruction, as in decode.py:119-128, 156-189: an "I" header at a P / B position
 * is decoded as plain intra, a "P" header at a B position predicts from the structure's first reference; a header type that
 * needs MORE references than the structure gives (the reference: IndexError) is CCD_ERR_VALUE. */
int ccd_get_coding_structure(const ccd_video_header* h, int32_t* display_order, int32_t* frame_type, int32_t* refs, int32_t* depth);

/* ---- one cool-chic: encode_decode_coolchic(mode="decode"), coolchic.py:29-207 ------------- */
/* Decodes one cool-chic on `device` and writes the synthesis output [C][H][W] float32 (after the
 * final resize/crop, coolchic.py:187-192) to `out`, a device pointer if out_on_device else host.
 * Synchronous with respect to `stream` on return when out is a host pointer. */
int ccd_decode_coolchic(const uint8_t* cc_header, size_t n_hdr, const uint8_t* bytes_nn, size_t n_nn,
                        const uint8_t* bytes_latent, size_t n_lat, int device, void* stream,
                        float* out, int out_on_device);

/* ---- batches of cool-chics: the throughput API (one frame per slot, many frames in flight) --
 * A batch owns the device-resident inputs (bitstream words, network parameters) and all
 * intermediate buffers of its slots.  Typical use: create, add every cool-chic of a set of
 * frames, then repeatedly run() - all slots decode concurrently (one workgroup per slot walks
 * the serial ARM + range-decoder chain; upsampling/synthesis tiles fill the rest of the chip). */
typedef struct ccd_batch ccd_batch;

int ccd_batch_create(int device, ccd_batch** out);
void ccd_batch_destroy(ccd_batch* b);
/* Adds one cool-chic; parses headers + network on the host and uploads to HBM. Returns the slot
 * index (>= 0) or an error.  bitdepth/frame_data_type describe the frame it belongs to and drive
 * the integer output planes (decode.py:191-206); pass bitdepth 0 to skip integer planes. */
int ccd_batch_add(ccd_batch* b, const uint8_t* cc_header, size_t n_hdr, const uint8_t* bytes_nn, size_t n_nn,
                  const uint8_t* bytes_latent, size_t n_lat, int bitdepth, int frame_data_type);
/* A slot whose latent grids are GIVEN instead of range-coded: no entropy work is launched for it.  What a caller that holds
 * candidate latents and networks (an encoder's search, a test pass) needs to see the planes they decode to, without writing a
 * payload (ccd_enc_run) and entropy-decoding it again.  `arch`, `bytes_nn` and `latents` are those of ccd_enc_add: the
 * transmitted fields of `arch` are read, latents[g] = int8 [grid_h[g]][grid_w[g]], index 0 the finest grid; bitdepth and
 * frame_data_type are those of ccd_batch_add.  Returns the slot index.
 * The slot is parsed, planned and run like a coded one (same float kernels, same options, same final resize, same planes bit
 * for bit as the coded slot that holds these latents); its header (ccd_batch_header) has n_bytes_latent = 0.  The grids sit
 * where the entropy kernel would have left them: ccd_batch_latent / ccd_batch_copy_latent work as for any slot.
 *   on_device == 0  host pointers, read during the call.  A value outside the coder's alphabet [-64, 63] is CCD_ERR_VALUE
 *                   and no slot is created.  The grids are uploaded with the slot's other inputs.
 *   on_device != 0  device pointers.  They are remembered and the grids are read EVERY time the batch runs (one copy launch
 *                   at the head of ccd_batch_run / ccd_batch_run_stage(.., 0), on the caller's stream), so a caller that
 *                   changes its latents in place and runs again sees the new planes, and nothing crosses PCIe.  The
 *                   pointers must stay valid while the batch may run: the contract of ccd_enc_add(..., 1), and the
 *                   lifetime rule of the note on ccd_batch_plane pointers at ccd_pool_trim.  A value outside [-64, 63]
 *                   makes ccd_batch_wait report CCD_ERR_VALUE for that slot (its planes are then unspecified and never
 *                   handed out by the copies); the other slots are unaffected, and the status is CCD_OK again after a run
 *                   that found the latents repaired.
 * ccd_batch_entropy_launches counts coded slots only (0 for a batch of given slots); coded and given slots may share a
 * batch.  ccd_batch_slot_stats words [1..3] are 0 for a given slot.  NULL b / arch / bytes_nn / latents and a bad bitdepth
 * are CCD_ERR_ARG, found before anything else is looked at; a NULL latents[g] is CCD_ERR_ARG, an `arch` that does not
 * re-parse CCD_ERR_VALUE. */
int ccd_batch_add_latents(ccd_batch* b, const ccd_cc_header* arch, const uint8_t* bytes_nn, size_t n_nn,
                          const int8_t* const* latents, int on_device, int bitdepth, int frame_data_type);
int ccd_batch_size(const ccd_batch* b);
int ccd_batch_header(const ccd_batch* b, int slot, ccd_cc_header* h);
/* Optional: builds and uploads the launch tables of the slots added so far (entropy descriptors, work lists of the float
 * kernels: one staged copy on `stream`) without launching anything - what the first ccd_batch_run[_stage] after an add does
 * anyway.  A caller that makes `stream` wait for other work (e.g. the decode of the batch before) calls this first, so that
 * the copy is not queued behind that wait. */
int ccd_batch_prepare(ccd_batch* b, void* stream);
/* Enqueues the whole decode of every slot on `stream` (asynchronous).  The entropy launches of a batch (one per kernel
 * instantiation and chain group: slots grouped by the expected length of their serial chains) fork over device-owned side
 * streams; each is followed on its own stream by the float-path launches of ITS frames, and everything joins on `stream`
 * before the call's remaining launches - so whatever is enqueued on `stream` afterwards sees every slot decoded
 * (CCD_OPT_OVERLAP = 0: float stages only behind the join, as three ccd_batch_run_stage calls would do).
 * ccd_batch_prepare and ccd_batch_run[_stage] may use different streams: a run orders itself behind the tables' copy. */
int ccd_batch_run(ccd_batch* b, void* stream);
/* Enqueue only one stage (profiling / tests): 0 entropy, 1 upsampling, 2 synthesis(+integer planes). */
int ccd_batch_run_stage(ccd_batch* b, void* stream, int stage);
/* Waits for `stream` - and, where that is another one, for the stream of the last ccd_batch_run[_stage]: the results are behind
 * the run - and returns the first per-slot decode error (CCD_ERR_INVALID_DATA ...).  The waits of the other handles
 * (ccd_enc_wait, ccd_dsens_wait, ccd_rdoq_wait, ccd_iscore_wait, ccd_quality_finish_batch, ccd_png_finish[_batch]) do the same. */
int ccd_batch_wait(ccd_batch* b, void* stream);
int ccd_batch_slot_status(const ccd_batch* b, int slot);
/* Raw per-slot counters of the entropy kernel after ccd_batch_wait: [0] status, [1] payload words read,
 * [2..3] symbols decoded (lo, hi); [36] latent grids whose body the pipelined kernel decoded as one stream of pixels
 * (batches cut without regard to wavefront steps: DESIGN.md 4.1); [37] batches its decoder took part by part; [39] pixels it
 * redid in int64 (dynamic operand check; with CCD_OPT_MFMA_ARM: 8-pixel tasks redone for an activation beyond three digits); [62] symbols that left the decoder's common path (window misses, sentinels), [63] of
 * which took the full 128-way search (pipelined kernel); the other words [4..61] are profiling cycle counters when built with
 * -DCCD_PIPE_PROFILE (which also reuses [36] and [37]).
 * `out64` receives 64 words. */
int ccd_batch_slot_stats(const ccd_batch* b, int slot, int32_t* out64);
/* Host only (tests): the chain groups ccd_batch_run would make of n slots with expected chain lengths est[] (any unit) and kernel
 * instantiations inst[] (0 .. k - 1; -1 = generic kernel) on a device with n_conc concurrent streams and n_cu CUs: cg[i] in 0 .. 2;
 * returns the number of groups in use.  See ccd_batch_run. */
int ccd_debug_chain_groups(const double* est, const int32_t* inst, int n, int n_conc, int n_cu, int32_t* cg);
/* Host only (tests): the entropy stage's walk over one grid of h x w latents, computed by the code the kernels and both
 * writers compile (ccd_wavefront.hpp).  which = 0: StepWalk::next from init; 1: StepIter::next; 2: for every step c >= 1 of
 * a wavefront grid, StepWalk::seek_before(c) followed by next() (step 0 from init); 3: the free functions, step by step;
 * 4: for every step c of a wavefront grid, the state of step c as seek_before(c + 1) leaves it (n: len_of, moved: moved_at).
 * steps (may be NULL): [cap][5] = y0, x0, n, moved, left after the step (moved / left: 0 where `which` has none).
 * segs (may be NULL): [3][6] = first, steps, pix_before, n_pix, task_pix, body of grid_segments(h, w, task_pix); *n_segs.
 * Returns the number of steps (also with steps == NULL), CCD_ERR_ARG for h, w < 1 or > 16383 or task_pix not 2 / 4 / 8. */
int64_t ccd_debug_grid_walk(int h, int w, int task_pix, int which, int32_t* steps, int64_t cap, int32_t* segs, int32_t* n_segs);
int ccd_debug_stream_min_step(void);   /* kStreamMinStep of this build */
/* How many of the library's side streams on `device` were MEASURED to run kernels concurrently (1 .. 4; once per process, ~10 ms
 * at the first call or the first ccd_batch_create): HIP multiplexes streams onto a few hardware queues, and launches on streams
 * that share one run one after the other.  The entropy launches of a batch that should overlap are put on these streams only,
 * and a batch is never split into more launches than that (environment: CCD_SIDE_STREAMS=k skips the measurement). */
int ccd_concurrent_streams(int device);
/* With CCD_OPT_TIME_LAUNCHES: duration in ms of every entropy launch of the LAST run (in launch order: longest expected chains
 * first) and the number of streams each holds; waits for those launches.  Returns the number of launches written (<= cap),
 * 0 when the option is off. */
int ccd_batch_launch_ms(ccd_batch* b, float* ms, int* n_streams, int cap);
/* Entropy launches per run of the batch as its launch tables were last built (ccd_batch_prepare / the first run after an add):
 * one per kernel instantiation in use and chain group (see ccd_batch_run); 0 before the tables exist. */
int ccd_batch_entropy_launches(const ccd_batch* b);
/* Which kernels serve this slot: bit 0 = pipelined entropy kernel (else the generic int64 one),
 * bit 1 = fused synthesis kernel (else one launch per layer), bit 2 = the whole float path (upsampling +
 * synthesis + integer samples) in one kernel, ccd_fused.hip, bit 3 = the ARM's layers evaluated on the matrix cores
 * inside the pipelined entropy kernel (exact limb-split int8, ccd_entropy_pipe.hip), bit 4 = the pipelined kernel's
 * instantiation that checks the IFCE features on the device (networks whose worst-case feature does not fit 16 bits),
 * bit 5 = the pipelined kernel's instantiation with a compile-time ARM shape (intra/hop.cfg: 14 + 6 inputs, two hidden layers),
 * bit 6 = the fused float kernel runs behind the batch's pyramid launch (CCD_OPT_FUSED_DEC = 2),
 * bit 7 = the network is OUTSIDE the finite envelope of the float stages (some latents could drive an intermediate value of the
 *         pyramid or the synthesis beyond float32: crafted or corrupt parameter payloads) - such a slot never runs the
 *         matrix-core kernel (bit 2 clear) but the vector-ALU kernels, which stay bit-identical with the reference
 *         arithmetic for inf and propagate NaN like torch.relu,
 * bit 8 = the latents were given (ccd_batch_add_latents): no entropy kernel serves the slot, bits 0, 3, 4, 5 are clear. */
int ccd_batch_slot_kernels(const ccd_batch* b, int slot);

/* Batch options, to be set before the slots they concern are added:
 *   CCD_OPT_FUSED_DEC   2 (default): slots whose architecture the fused float kernel covers (every decoder preset of
 *                       the reference, cfg/dec) run it behind ONE pyramid launch per batch that evaluates the latent
 *                       levels >= 1 once per frame (stage 1); the fused kernel's tiles load their level-1 footprint and do
 *                       level 0 + synthesis + integer samples (stage 2).  1: the fused kernel alone, the whole pyramid per
 *                       tile (one launch, nothing but the int8 latents read; ~20 % slower).  0: unfused path (per-level
 *                       upsampling launches + synthesis kernel), which materialises the dense stack ccd_batch_dense()
 *                       returns.  The three produce the same bits.
 *   CCD_OPT_KEEP_FLOAT  1 (default): the f32 synthesis output is always written (ccd_batch_output);
 *                       0: slots that produce integer planes directly (rgb / yuv444 intra frames) write only those.
 *   CCD_OPT_MFMA_ARM    0 (default): the integer ARM on the vector ALU; 1: streams inside the envelope (<= 20 ARM inputs,
 *                       <= 8 IFCE features, |weight| <= 0x7F7F7F, worst-case IFCE feature <= 0x7F7F, widest grid <= 2 500)
 *                       evaluate it with v_mfma_i32_16x16x64_i8 (exact: operands split into signed-digit bytes, three per
 *                       weight and activation, two per feature - hence the limits).  Results are identical bit for bit
 *                       either way; on MI355X the matrix-core variant is the slower one, it is kept as a
 *                       measured alternative.  A task that meets a hidden activation above 0x7F7F7F is redone in plain
 *                       int64; values 2..22 lower that limit to 2^value so that tests reach the redo with ordinary streams.
 *   CCD_OPT_RANGE_BITS  0 (default): production limit of the pipelined entropy kernel's dynamic operand check (an IFCE feature
 *                       with |f| >= 2^15 sends its pixel through the int64 redo).  Tests pass 8..14 to lower the limit and
 *                       drive ordinary streams through the redo; results are identical bit for bit.
 *                       ccd_batch_slot_stats word [39] counts the redone pixels; word [37] counts the batches the
 *                       pipelined kernel's decoder took part by part (a producer task at a time, because only the first
 *                       part's tables were there when it looked: DESIGN.md 4.1).
 *   CCD_OPT_OVERLAP     1 (default): ccd_batch_run overlaps the float path of the streams that finish early with the longest
 *                       entropy chains (chain groups, see ccd_batch_run); 0: one entropy launch per kernel instantiation and
 *                       every float launch behind the join.  Results are identical bit for bit (A/B, tests).  Environment:
 *                       CCD_OVERLAP=0.
 *   CCD_OPT_TIME_LAUNCHES  0 (default); 1: timing events around every entropy launch on the stream it runs on; ccd_batch_launch_ms
 *                       returns the durations of the last run (measurement only: bench.py's roofline). */
enum { CCD_OPT_FUSED_DEC = 1, CCD_OPT_KEEP_FLOAT = 2, CCD_OPT_MFMA_ARM = 3, CCD_OPT_RANGE_BITS = 4, CCD_OPT_OVERLAP = 5, CCD_OPT_TIME_LAUNCHES = 6 };
int ccd_batch_set_option(ccd_batch* b, int option, int value);

/* Device pointers of a slot's results (valid until the batch is destroyed / re-run): */
const float* ccd_batch_output(const ccd_batch* b, int slot);    /* [C][H][W] f32, synthesis output */
const float* ccd_batch_dense(const ccd_batch* b, int slot);     /* [L][H0][W0] f32, Upsampling.forward; NULL on the fused path */
const int8_t* ccd_batch_latent(const ccd_batch* b, int slot, int grid); /* [h][w] int8 */
/* Integer planes (value = round(x * (2^bitdepth-1)) after the reference's clamp/round/420 chain):
 * plane p of the frame, uint8 if bitdepth == 8 else uint16; chroma planes are half size for yuv420. */
const void* ccd_batch_plane(const ccd_batch* b, int slot, int plane, int* h, int* w);
/* Copies (device -> host, synchronous on `stream`) for tests and writers. */
int ccd_batch_copy_latent(ccd_batch* b, int slot, int grid, int8_t* host, void* stream);
int ccd_batch_copy_plane(ccd_batch* b, int slot, int plane, void* host, void* stream);
int ccd_batch_copy_output(ccd_batch* b, int slot, float* host, void* stream);
int ccd_batch_copy_dense(ccd_batch* b, int slot, float* host, void* stream);
/* The writer's path (decode.py:84-89 hands every frame to a file writer): a slot's three integer planes sit in ONE block of
 * device memory, plane p at byte offset off3[p] (256-byte aligned) of total_bytes.  ccd_batch_copy_planes_async enqueues one
 * device -> host copy per slot of [first_slot, first_slot + n_slots) into host_blocks[i] (same layout; pinned memory makes
 * them true DMA transfers) and returns without waiting: the caller waits on `stream` (ccd_batch_wait).  A slot whose decode
 * failed is skipped and its error returned. */
int ccd_batch_planes_layout(const ccd_batch* b, int slot, size_t* total_bytes, size_t* off3);
int ccd_batch_copy_planes_async(ccd_batch* b, int first_slot, int n_slots, void* const* host_blocks, void* stream);
/* Device and pinned-host blocks of destroyed batches are cached per device for the next batch (a batch per image set is the
 * normal use); this returns them to the runtime.  The environment variables CCD_POOL_MAX_MB / CCD_PINNED_POOL_MAX_MB cap the
 * caches of EACH device (defaults 16384 / 2048 MB per device = 5.5 % of it: the cache is invisible to other allocators of the process, e.g. PyTorch's; a block beyond
 * the cap is freed at once, and an allocation that fails trims the cache and retries).
 *
 * Threading and global state.  Per device and for the life of the process the library keeps: that block cache, the two
 * Laplace tables, ONE upload stream and eight side streams (entropy launches of one batch that need different kernel
 * instantiations - or hold streams of very different lengths - fork onto those of them that were measured to run concurrently,
 * ccd_concurrent_streams, and join the caller's stream again).  All of it is created under a lock; the fork / join
 * events belong to the batch.  Different batches may be driven from different host threads on one device; ONE batch is not
 * thread-safe.  ccd_batch_destroy drains every stream the caller passed to ccd_batch_run[_stage], ccd_batch_wait and
 * ccd_batch_copy_* before the batch's blocks return to the cache; work the caller enqueued on OTHER streams that reads
 * pointers obtained from ccd_batch_plane / _output / _latent must be finished by the caller before the destroy.  A stream
 * handed to any ccd_batch_* call must stay alive until the batch is destroyed (the destroy synchronises it). */
void ccd_pool_trim(int device);

/* ---- whole file: decode_video(), decode.py:26-91 ----------------------------------------- */
typedef struct {
    int32_t display_index, frame_type, frame_data_type, bitdepth;
    int32_t h, w, ch, cw;
    uint16_t* plane[3]; /* host, malloc'ed by the library, integer samples (u16 for every bitdepth) */
} ccd_frame;

typedef struct {
    int32_t n_frames;
    ccd_frame* frames; /* display order */
} ccd_video;

int ccd_decode_video(const uint8_t* bitstream, size_t n, int device, ccd_video* v);

/* ---- P / B frame reconstruction: decode.py:156-206 ------------------------------------------- */
/* All pointers are DEVICE pointers. residue = synthesis output of the "residue" cool-chic ([4][h][w] for P,
 * [5][h][w] for B: rgb/yuv residue, alpha, beta), motion = output of the "motion" cool-chic ([2] or [4][h][w]:
 * (x, y) flow per reference), refN_planes = the three integer planes of each reference frame (u8 if
 * bitdepth == 8 else u16; half-size chroma for yuv420), global_flow = (x, y) integer translation per reference
 * (frame header), warp_filter_size = 2 (bilinear) / 4 (bicubic grid_sample) / 6..16 even (sinc) as in warp.py:49-56.  Writes the integer planes of the frame.
 * CCD_ERR_ARG for a missing buffer or a bit depth outside 8..16, CCD_ERR_VALUE for a filter size or frame_data_type (0..3) out of
 * range and for yuv420 with an odd h or w; all checked before the device is touched.
 * The launches go to `stream` and read the inputs in stream order; the call synchronises `stream` before it returns (its scratch
 * goes back to the block cache), so the planes are written on return. */
int ccd_inter_reconstruct(int device, void* stream, int frame_type, int h, int w, int bitdepth, int frame_data_type,
                          const float* residue, const float* motion, const void* const* ref0_planes,
                          const void* const* ref1_planes, const int32_t* global_flow, int warp_filter_size,
                          void* const* out_planes);
void ccd_video_free(ccd_video* v);

/* ---- bitstream writer + synthetic streams ("next-2" row of SURVEY section 8f) -------------- */
/* Range-encodes `n` symbols with per-symbol (mu_idx, scale_idx) table indices exactly as
 * constriction 0.4.2's RangeEncoder + QuantizedLaplace(-64,63) (rangecoder.py:46-76).
 * Returns the number of bytes written to *out (malloc'ed; free with ccd_free). */
int64_t ccd_range_encode(const int8_t* symbols, const int32_t* mu_idx, const int32_t* scale_idx, int64_t n,
                         uint8_t** out);
/* Bitstream writer for one intra frame (bitstream/encode.py:24-95): frames the video / frame /
 * cool-chic headers (architecture = the transmitted fields of `tmpl`), the NN payload `bytes_nn`
 * verbatim and the range-coded `latents` (latents[g] = int8 [grid_h[g]][grid_w[g]], values in
 * [-64, 63]).  The encoder walks the decoder's integer ARM/IFCE path on the HOST, like the
 * reference (latent.py:168-173).  Used by bench.py and the round-trip tests to manufacture
 * Kodak/CLIC/4K-shaped inputs; never used while decoding. */
int64_t ccd_encode_stream(const ccd_cc_header* tmpl, const uint8_t* bytes_nn, size_t n_nn,
                          const int8_t* const* latents, int bitdepth, int frame_data_type, uint8_t** out);
/* The cool-chic part alone (cool-chic header + NN payload + range-coded latents), for multi-frame /
 * multi-cool-chic streams assembled by the caller (bitstream/encode.py:83-92). */
int64_t ccd_encode_coolchic(const ccd_cc_header* tmpl, const uint8_t* bytes_nn, size_t n_nn,
                            const int8_t* const* latents, uint8_t** out);
/* Number of transmitted integers per (module, weight|bias) group for the architecture in `arch` (only the
 * transmitted fields are read), order arm.w arm.b ifce.w ifce.b ups.w ups.b syn.w syn.b
 * (component/core/types.py:18-19,98-101; neuralnet.py:46-71). */
int ccd_network_layout(const ccd_cc_header* arch, int64_t n_values[8]);
/* Exp-Golomb NN payload writer: encode_network + encode_exp_golomb (neuralnet.py:27-90, expgolomb.py:15-71).
 * `values` = the quantised parameters in stream order, orders taken from arch->nn_expgol_cnt.  Returns the
 * byte count (malloc'ed *out, free with ccd_free); *n_bit_pad = prefix padding bits for the header. */
int64_t ccd_encode_network(const ccd_cc_header* arch, const int32_t* values, int64_t n_values, int32_t* n_bit_pad,
                           uint8_t** out);
/* ---- network quantisation (host only; cool_chic_amd/nnquant.py) --------------------------------
 * The transmitted integers of an NN payload in stream order (the groups of ccd_network_layout, Exp-Golomb orders and padding
 * from `arch`): what ccd_encode_network takes.  Returns their number; CCD_ERR_ARG when `cap` is smaller, CCD_ERR_VALUE for an
 * integer outside int32, else what the payload parser refuses. */
int64_t ccd_network_values(const ccd_cc_header* arch, const uint8_t* bytes_nn, size_t n_nn, int32_t* values, int64_t cap);
/* The header's table of quantisation steps of group 0 .. 7 (nnquant/quantstep.py:26-43): returns its length n and sets
 * *log2_first; the steps are 2^(*log2_first) .. 2^(*log2_first + n - 1).  CCD_ERR_ARG for another group or a null pointer. */
int ccd_q_step_table(int group, int32_t* log2_first);
/* values[i] = rint(x[i] / 2^q_step_log2[group of i]) in float32, ties to even (torch.round(x / q); the division by a power of
 * two is exact): float parameters in stream order -> the integers a decoder multiplies by the same steps.  CCD_ERR_VALUE for
 * a step outside the header's table of its group (counts 9 17 9 17 13 1 13 25 from log2 -8 -16 -8 -16 -12 0 -12 -24), for a
 * non-finite x and for a result outside int32; CCD_ERR_ARG when n_values is not the layout's total. */
int ccd_quantise_network(const ccd_cc_header* arch, const float* x, int64_t n_values, const int32_t q_step_log2[8],
                         int32_t* values);
/* Per group the Exp-Golomb order 0 .. 12 whose code of the group's values is shortest (counted, ties to the smaller order,
 * 0 for an empty group) and that length in bits: an encode with these orders has ceil(sum of n_bits / 8) bytes. */
int ccd_network_best_expgol(const ccd_cc_header* arch, const int32_t* values, int64_t n_values, int32_t order[8],
                            int64_t n_bits[8]);
/* Header writers, AbstractHeader.to_bytes (header.py:90-105); n_bytes_header is computed. Return bytes written. */
int ccd_write_cc_header(const ccd_cc_header* h, uint8_t* out, size_t cap); /* transmitted fields only */
int ccd_write_frame_header(const ccd_frame_header* f, uint8_t* out, size_t cap);
int ccd_write_video_header(const ccd_video_header* v, uint8_t* out, size_t cap);
void ccd_free(void* p);

/* ---- PNG packing on the device (reference: coolchic/io/format/png.py:44-62 write_png, which hands an HWC uint8
 * array to PIL / zlib on the host).  r, g, b: device pointers to [h][w] uint8 planes (ccd_batch_plane); out: device
 * buffer, 4-byte aligned, of at least ccd_png_bound(h, w) bytes.  ccd_png_pack only enqueues work on `stream`;
 * ccd_png_finish synchronises the stream and returns the size of the file in `out` (or a negative code).  One pack
 * (single or batch) may be in flight per handle.  The file holds the filtered scanlines in dynamic-Huffman deflate
 * blocks: any PNG reader decodes exactly the input planes; the bytes differ from PIL's (PNG bytes are not normative).
 * Level CCD_PNG_LITERAL (0, the default of a new handle): literal-only blocks.  Level CCD_PNG_LZ77 (1): every block
 * also searches matches inside itself (LZ77 on the device) and keeps the level-0 coding where
 * that is not smaller, so a level-1 file is never larger than the level-0 file and ccd_png_bound still holds.
 * ccd_png_destroy frees the workspace with hipFree, which waits for the device: a pack still in flight on any stream has
 * finished when it returns. */
typedef struct ccd_png ccd_png;
typedef struct {
    const uint8_t *r, *g, *b; /* device planes [h][w] */
    int32_t h, w;
    uint8_t* out;             /* device buffer, 4-byte aligned */
    size_t cap;               /* >= ccd_png_bound(h, w) */
} ccd_png_item;
size_t ccd_png_bound(int h, int w);  /* 0 if a side is outside 1..16383 */
int ccd_png_create(int device, ccd_png** out);
void ccd_png_destroy(ccd_png* p);
int ccd_png_pack(ccd_png* p, const uint8_t* r, const uint8_t* g, const uint8_t* b, int h, int w, uint8_t* out,
                 size_t cap, void* stream);
int64_t ccd_png_finish(ccd_png* p, void* stream);
/* Many pictures in one set of launches (every deflate block of every picture is a workgroup of the same kernels);
 * ccd_png_finish_batch synchronises the stream and fills sizes[n] (n = the count given to the pack). */
int ccd_png_pack_batch(ccd_png* p, const ccd_png_item* items, int n, void* stream);
int ccd_png_finish_batch(ccd_png* p, void* stream, int64_t* sizes, int n);
/* Level of the packs enqueued from now on (a pack already in flight is unaffected).  CCD_ERR_ARG for a NULL handle or
 * a level other than CCD_PNG_LITERAL / CCD_PNG_LZ77. */
enum { CCD_PNG_LITERAL = 0, CCD_PNG_LZ77 = 1 };
int ccd_png_set_level(ccd_png* p, int level);

/* ---- bitstream writer on the device (reference: bitstream/encode.py:83-92, component/latent.py:142-173; DESIGN.md
 * section 4.10).  Turns (architecture, NN payload, latent grids) into exactly the bytes ccd_encode_coolchic returns: the
 * contexts of every pixel of every grid are evaluated at once (the encoder knows all latents), then one wave per slot runs
 * the range encoder's interval chain.  All slots of a handle are encoded by the same two launches.
 * ccd_enc_add: latents[g] = int8 [grid_h[g]][grid_w[g]], host pointers (copied at add; a value outside [-64, 63] is
 * CCD_ERR_VALUE) or, with latents_on_device != 0, device pointers such as ccd_batch_latent() returns (read when a run
 * EXECUTES, so they must stay valid; a value outside [-64, 63] makes ccd_enc_wait return CCD_ERR_VALUE for that slot, the
 * other slots are unaffected).  Returns the slot index.  NULL arguments are CCD_ERR_ARG, a template that does not re-parse
 * CCD_ERR_VALUE; both are found before the device is touched.
 * ccd_enc_run only enqueues on `stream`; ccd_enc_wait synchronises and returns the first per-slot error.  One run may be in
 * flight per handle; a handle can be run again (same bytes) and can take more slots after a run.  ccd_enc_destroy drains
 * the streams the handle was given. */
typedef struct ccd_enc ccd_enc;
int ccd_enc_create(int device, ccd_enc** out);
void ccd_enc_destroy(ccd_enc* e);
int ccd_enc_add(ccd_enc* e, const ccd_cc_header* tmpl, const uint8_t* bytes_nn, size_t n_nn, const int8_t* const* latents,
                int latents_on_device);
int ccd_enc_size(const ccd_enc* e);
int ccd_enc_run(ccd_enc* e, void* stream);
int ccd_enc_wait(ccd_enc* e, void* stream);
/* After wait: cool-chic header (n_bytes_latent filled in) + NN payload + range-coded latents, == ccd_encode_coolchic;
 * malloc'ed *out, free with ccd_free.  Returns the byte count, the slot's error, or CCD_ERR_ARG (bad slot, no finished run). */
int64_t ccd_enc_slot_bytes(ccd_enc* e, int slot, uint8_t** out);
/* The range-coded payload where it was written: device pointer (4-byte aligned) and size in bytes, valid until the next
 * run / destroy - what a decoder or verifier on the same GPU reads without a copy through the host. */
int64_t ccd_enc_slot_payload(const ccd_enc* e, int slot, const uint8_t** device_ptr);
/* After wait: the slot's status; out8 (optional) receives [0] status, [1] payload words, and how the coder's carry was
 * exercised: [2] "inverted" runs begun (the interval straddled 2^64 at a word boundary), [3] runs resolved with a carry,
 * [4] resolved without one. */
int ccd_enc_slot_status(const ccd_enc* e, int slot, int32_t* out8);
/* ---- rate meter: what a slot's latents cost under its ARM, without the range coder's serial chain.
 * A symbol whose interval is (left, right) out of 2^24 costs 24 - log2(right - left) bits; a measure evaluates every
 * interval like a run does and sums per latent grid, in float64, in an order that depends only on the grid's size: a slot
 * gives the same 64 bits alone and inside any batch.  sum_width is the exact integer sum of (right - left) over the grid.
 * ccd_enc_measure only enqueues on `stream`; it counts as the handle's one run in flight: ccd_enc_wait ends it and returns
 * the first per-slot error, ccd_enc_destroy drains it.  want_map != 0 also leaves float32 bits of every latent on the device.
 * Results of a measure and of a run live in separate buffers: a later ccd_enc_run does not invalidate ccd_enc_slot_rate, a
 * later ccd_enc_measure does not invalidate ccd_enc_slot_bytes / _payload / _status.
 * ccd_enc_slot_rate: the slot's status (0, or CCD_ERR_VALUE for a device latent outside [-64, 63]: out->status says the same
 * and no numbers are reported; the other slots are unaffected); CCD_ERR_ARG for a NULL handle or `out`, a bad slot, or a slot
 * no finished measure covered.
 * ccd_enc_slot_rate_map: device pointer to grid_h[grid] * grid_w[grid] floats in raster order and their count; valid until
 * the next measure / destroy.  CCD_ERR_ARG when the last measure had want_map == 0, for a bad slot or grid, a NULL argument.
 * NULL handles are found before the device is touched. */
typedef struct {
    int32_t status;                      /* 0 or the slot's error */
    int32_t n_grids;
    int64_t n_symbols[CCD_MAX_GRIDS];
    uint64_t sum_width[CCD_MAX_GRIDS];   /* exact: sum of (right - left) over the grid */
    double bits[CCD_MAX_GRIDS];          /* sum of 24 - log2(width) over the grid */
    double total_bits;                   /* sum of bits[] in grid order 0 .. n_grids - 1, added on the device */
    int64_t n_bytes_nn, n_bytes_header;  /* what the slot's other bytes are: known at add */
} ccd_enc_rate;
int ccd_enc_measure(ccd_enc* e, void* stream, int want_map);
int ccd_enc_slot_rate(const ccd_enc* e, int slot, ccd_enc_rate* out);
int64_t ccd_enc_slot_rate_map(const ccd_enc* e, int slot, int grid, const float** device_ptr);
/* ---- rate sensitivity: the exact change of a slot's model bits if ONE latent were v - 1 or v + 1 (DESIGN.md section 4.10,
 * "Rate sensitivity").  Changing the latent p changes its own interval, the intervals of the later pixels of its grid that
 * hold it in their spatial context and those of the finer-grid pixels whose IFCE feature reads it; the map holds the sum of
 * 24 - log2(width) over exactly those pixels with the changed latent, minus the same sum with the latents as they are.
 * ccd_enc_measure_deltas is a ccd_enc_measure(e, stream, 0) - same ccd_enc_slot_rate results, word for word, same rule of
 * one operation in flight, ended by ccd_enc_wait - followed by the two delta launches.
 * Its own buffers are taken before anything is enqueued: CCD_ERR_NOMEM / CCD_ERR_UNSUPPORTED leave the handle idle.
 * ccd_enc_slot_delta_map: device pointer to float32 [2][grid_h][grid_w] (plane 0: v - 1, plane 1: v + 1; +inf where the move
 * leaves [-64, 63]) and grid_h * grid_w; valid until the next measure, measure_deltas or destroy (a run does not touch it).
 * A slot with a latent outside the alphabet has the status CCD_ERR_VALUE, which is returned in place of a map.  CCD_ERR_ARG for
 * a NULL argument, a bad slot or grid, or when the last finished measure was not a measure_deltas that covered the slot. */
int ccd_enc_measure_deltas(ccd_enc* e, void* stream);
int ccd_enc_slot_delta_map(const ccd_enc* e, int slot, int grid, void** dev_ptr);
/* ---- ARM parameter deltas: the exact change of a slot's model bits if ONE transmitted integer of its ARM were v - 1 or v + 1
 * (DESIGN.md section 4.20).  Parameter k, 0 <= k < ccd_enc_slot_param_count, counts the ARM's integers in stream order
 * (ccd_network_values: groups 0 and 1 of ccd_network_layout): the weights of every layer [out][in], the stabiliser's [2][dim],
 * then the biases of every layer and the stabiliser's two.  The candidate network is the slot's with values[k] + s taken
 * through the fixed-point conversion ccd_enc_add applies; per (k, s), s = -1 first:
 *   bits       float64  total_bits with the candidate - total_bits as it is: the sum over the symbols whose interval width
 *                       changed of log2(width) - log2(width'); exactly 0.0 when none did
 *   sum_width  int64    the exact change of the meter's sum_width (over all grids)
 *   moved      int64    the number of symbols whose width changed
 * A candidate whose integer leaves int32 cannot be transmitted: +inf, 0, 0.
 * ccd_enc_measure_param_deltas is a ccd_enc_measure(e, stream, 0) - same ccd_enc_slot_rate results, word for word, same rule of
 * one operation in flight, ended by ccd_enc_wait - followed by the table's two launches for the parameters [first, first + count)
 * of every slot (count < 0: all from first; the range is clipped to each slot's parameter count).  A slot's words do not depend
 * on the range, the other slots, the device or the mode.  mode: 0 automatic (the incremental path where a slot's state fits the
 * LDS, else the generic one), 1 the generic path (one full evaluation of the model per candidate and symbol), 2 the incremental
 * path (the base evaluation's accumulators kept per lane, a candidate as a rank-1 update of the layer behind it): if a slot's
 * state does not fit, the call returns CCD_ERR_UNSUPPORTED.  CCD_ERR_ARG (NULL handle, first < 0, another mode) and
 * CCD_ERR_UNSUPPORTED (mode 2 as above; more than 65 535 slots or 2 x 2^21 candidates of one slot in a call) are found before
 * the device is touched and leave the handle and the last table as they were; CCD_ERR_NOMEM / CCD_ERR_HIP leave no table.
 * ccd_enc_slot_param_deltas: the slot's range into *first / *count and the three arrays [count][2] (any of the five may be
 * NULL); returns the slot's status like ccd_enc_slot_delta_map (CCD_ERR_VALUE for a device latent outside the alphabet, nothing
 * is written then).  CCD_ERR_ARG for a NULL handle, a bad slot, or when the last finished measure was not a
 * measure_param_deltas that covered the slot: the next measure of any kind invalidates the table, a run does not touch it. */
int ccd_enc_measure_param_deltas(ccd_enc* e, void* stream, int first, int count, int mode);
int ccd_enc_slot_param_count(const ccd_enc* e, int slot);
int ccd_enc_slot_param_deltas(const ccd_enc* e, int slot, int* first, int* count, double* bits, int64_t* sum_width, int64_t* moved);
/* ---- IFCE parameter deltas: the same table for the transmitted IFCE integers.  Parameter k,
 * 0 <= k < ccd_enc_slot_ifce_count, counts groups 2 and 3 of ccd_network_layout in stream order: the weights [n_ifce_out][fin_g]
 * of every grid with input_features_ifce[g] > 0 in grid order, then the biases [n_ifce_out] of those grids.  The fields, the
 * +inf, 0, 0 of a move that leaves int32, the range, the modes, the refusals and the rule that the next measure of any kind
 * invalidates the table are those of the three functions above; ccd_enc_measure_ifce_deltas is a ccd_enc_measure(e, stream, 0)
 * followed by the table.  A weight of the coarsest grid reads an all-zero channel: its rows are exactly 0.0, 0, 0.  A slot
 * without IFCE has ccd_enc_slot_ifce_count == 0 and an empty table (*count == 0), it refuses no mode.  A handle holds ONE table:
 * after a measure_ifce_deltas ccd_enc_slot_param_deltas returns CCD_ERR_ARG, and ccd_enc_slot_ifce_deltas after a
 * measure_param_deltas. */
int ccd_enc_measure_ifce_deltas(ccd_enc* e, void* stream, int first, int count, int mode);
int ccd_enc_slot_ifce_count(const ccd_enc* e, int slot);
int ccd_enc_slot_ifce_deltas(const ccd_enc* e, int slot, int* first, int* count, double* bits, int64_t* sum_width, int64_t* moved);
/* Size of a slot's payload buffer: every symbol has a width of at least 1 / 2^24, so n symbols give at most
 * 4 * (ceil(24 n / 32) + 2) bytes.  0 for n < 0. */
size_t ccd_enc_payload_bound(int64_t n_symbols);

/* ---- rate model (reference: coolchic/component/core/arm.py:448-485 compute_rate / _laplace_cdf, float32) ------
 * rate[i] = -log2(max(cdf(x+0.5) - cdf(x-0.5), 2^-16)) with the continuous Laplace(mu, scale) of the reference.
 * x, mu, scale, rate (optional), total_bits (optional, one double) are DEVICE pointers; asynchronous on `stream`.
 * x, mu, scale and rate are arrays of n floats each, at any 4-byte alignment (all four 16-byte aligned: the vector kernel);
 * exactly n floats of rate are written.  total_bits is overwritten (its value before the call does not matter) with the sum
 * of the n rates in float64; with n == 0 it becomes 0.0 and rate is not touched.  Both outputs may be asked for in one call.
 * NaN in, NaN out: a NaN in x[i], mu[i] or scale[i] gives rate[i] = NaN (never the 16 bits of the clamp) and a NaN total.
 * scale[i] is a positive normal float; for any other scale (zero, negative, subnormal, infinite), or an infinite x or mu, the
 * values are unspecified, but no memory access depends on the values.  CCD_ERR_ARG for a NULL x, mu or scale, n < 0, or both
 * outputs NULL (checked before the device is touched). */
int ccd_compute_rate(int device, void* stream, const float* x, const float* mu, const float* scale, int64_t n,
                     float* rate, double* total_bits);

/* ---- quality of decoded frames against their source, on the device -------------------------
 * Compares the integer planes of a batch of frames (ccd_batch_plane) with source planes of the same types and sizes in one
 * set of launches.  PSNR as the reference defines it (training/metrics/mse.py:14-21, loss.py:88-118): the squared error of
 * every plane as an exact 64-bit integer; the division and the logarithm happen on the host (ccd_quality_psnr).
 * MS-SSIM (Wang, Simoncelli, Bovik 2003) per plane on x = sample / (2^bitdepth - 1): 5 scales, 11-tap Gaussian window
 * (sigma 1.5) applied separably without padding, C1 = 0.01^2, C2 = 0.03^2, 2 x 2 mean with stride 2 between scales (a trailing
 * odd row or column is dropped); the device returns the spatial means of cs and ssim per scale, ccd_quality_ms_ssim
 * combines them.  A plane whose shorter side is below 176 has n_scales = 0 (its MS-SSIM is NaN): a result, not an error.
 * The results of a picture do not depend on what else is in the batch, and the same batch gives the same bits every time.
 * ccd_quality_score_batch only enqueues on `stream` (the planes must stay valid until the finish); ccd_quality_finish_batch
 * synchronises and fills results[n] (n = the count given to the score).  One scoring may be in flight per handle; a handle
 * is reusable; ccd_quality_destroy drains the streams the handle was given.  CCD_ERR_ARG - before the device is touched -
 * for a NULL argument, n <= 0, a bit depth outside 8..16, a side outside 1..16383, a `what` of 0 or with unknown bits. */
typedef struct ccd_quality ccd_quality;
typedef struct {
    const void* dec[3];      /* device planes, u8 if bitdepth == 8 else u16 (ccd_batch_plane) */
    const void* src[3];      /* device planes of the source, same types and sizes */
    int32_t h, w, ch, cw;    /* luma size, chroma size (== h, w unless yuv420) */
    int32_t bitdepth;        /* 8..16 */
} ccd_quality_item;
typedef struct {
    uint64_t sse[3], n[3];
    int32_t  n_scales[3];    /* 5, or 0 when the plane is too small (or MS-SSIM was not asked for) */
    double   cs[3][5], ssim[3][5];   /* spatial means per scale */
} ccd_quality_result;
enum { CCD_QUALITY_PSNR = 1, CCD_QUALITY_MS_SSIM = 2 };
int ccd_quality_create(int device, ccd_quality** out);
void ccd_quality_destroy(ccd_quality* q);
int ccd_quality_score_batch(ccd_quality* q, const ccd_quality_item* items, int n, int what, void* stream);
int ccd_quality_finish_batch(ccd_quality* q, void* stream, ccd_quality_result* results, int n);
/* Host only, no device needed.  psnr: -10 log10(sum sse / (sum n * maxv^2)) over one plane or, plane = -1, the whole frame
 * (+inf for identical pictures; NaN for a NULL result, a bad plane or bit depth).  ms_ssim: prod_{j<4} max(cs[j], 0)^w_j *
 * max(ssim[4], 0)^w_4 of one plane, NaN when n_scales is 0. */
double ccd_quality_psnr(const ccd_quality_result* r, int bitdepth, int plane);
double ccd_quality_ms_ssim(const ccd_quality_result* r, int plane);
/* Host only: validates like ccd_quality_score_batch (pointers are compared with NULL, never read) and returns the bytes of
 * device scratch the scoring takes from the block cache, or CCD_ERR_ARG. */
int64_t ccd_quality_scratch_bytes(const ccd_quality_item* items, int n, int what);

/* ---- distortion deltas: the exact change of a frame's squared error if ONE latent were v - 1 or v + 1
 * Take a candidate (arch, networks, latents) and a source frame.  For grid g, position (y, x) and sign s in {-1, +1}:
 *
 *     dD[s][g][y][x] = SSE(planes decoded with latent[g][y][x] + s, everything else unchanged)
 *                    - SSE(planes decoded with the latents as given)
 *
 * SSE is the sum over all three integer planes of (decoded - source)^2, the quality meter's definition (section 4.11); the
 * value is a signed 64-bit integer.  Where v + s leaves [-64, 63] the entry is INT64_MIN (the +inf of the rate deltas).  A
 * hyperlatent grid (is_hyperlatent[g]) does not feed the synthesis: its map is all zeros (the sentinel at the alphabet's ends)
 * and costs no passes.  Layout: int64 [2][h][w] per grid on the device, s = -1 first, like ccd_enc_slot_delta_map.
 * frame_data_type 0 rgb, 1 yuv420, 2 yuv444 at 8..16 bits.  ccd_dsens_add takes the one cool-chic of an intra frame,
 * ccd_dsens_add_inter one of the two of a P / B frame.
 *
 * No float arithmetic of its own: the planes of a moved latent come from given-latent slots of a decode batch the handle owns
 * (per candidate one base slot that reads the caller's latents and n_probe_slots slots that read private copies, all with
 * on_device = 1).  One pass of the float path moves every latent of one lattice (y % S == py, x % S == px) of one grid by s: the
 * stride S is wide enough that the samples two of them can change do not overlap, and the squared-error change inside a
 * probe's own box is its entry - the number one decode per latent would give.
 *
 * ccd_latent_footprint (host only): box = {top, left, bottom, right}, offsets in luma samples for the latent (0, 0) of `grid`.
 * A move of the latent (y, x) can only change the samples in rows [sy + top, sy + bottom] and columns [sx + left, sx + right],
 * clipped to the picture, where sy = floor(y * 2^l * img_size[0] / grid_h[g0]) and sx = floor(x * 2^l * img_size[1] / grid_w[g0]):
 * g0 is the finest latent grid (the resolution of the synthesis), l the number of latent grids finer than `grid` (the grid's
 * pixel pitch is 2^l when there is no final resize).  The 4:2:0 chroma planes take the box halved, rounded outwards.  Derived
 * from the supports of the filters alone; it may be conservative, never too small.  Returns 0; 1 for a
 * hyperlatent grid, which has no footprint (box = {0, 0, -1, -1}); CCD_ERR_ARG for NULL or a bad grid, CCD_ERR_VALUE for an
 * `arch` whose transmitted fields do not re-parse.
 * ccd_latent_probe_stride (host only): the stride S the passes of `grid` use for a frame of this frame_data_type: the smallest
 * for which the boxes (and, 4:2:0, the chroma boxes) of two latents S apart in either direction are disjoint.  0 for a
 * hyperlatent grid; errors as above, and CCD_ERR_ARG for a frame_data_type other than 0, 1, 2.
 *
 * ccd_dsens_add: `arch`, `bytes_nn` as for ccd_batch_add_latents; latents[g] = DEVICE int8 [grid_h[g]][grid_w[g]], read at
 * every run and never written; src[p] = DEVICE planes of the source (u8 if bitdepth == 8 else u16, half-size chroma for
 * yuv420), read at every run.  Both must stay valid while the handle may run.  Returns the slot index.  CCD_ERR_ARG - before
 * the device is touched - for a NULL argument (a NULL latents[g] or src[p] included), a bit depth outside 8..16, a
 * frame_data_type other than 0, 1, 2, a run in flight; CCD_ERR_VALUE for an `arch` that does not re-parse.
 * ccd_dsens_create: n_probe_slots outside 1..64 and a NULL `out` are CCD_ERR_ARG, found before the device is touched.  The
 * maps do not depend on n_probe_slots, nor on what else the handle holds.
 * ccd_dsens_run enqueues, on `stream`, rounds of up to n_probe_slots passes per candidate: apply (ccd_dsens.hip), ccd_batch_run,
 * squared-error split.  ccd_dsens_wait synchronises and returns the first per-slot error: a base latent outside [-64, 63] is
 * that slot's CCD_ERR_VALUE, the other slots are unaffected.  One run may be in flight per handle; a handle can be run again
 * (after the caller changed its latents in place, say) and can take more slots after a wait.
 * ccd_dsens_slot_map: device pointer to int64 [2][grid_h][grid_w] and grid_h * grid_w as the return value; valid until the next
 * run / destroy.  The slot's error in place of a map; CCD_ERR_ARG for a NULL argument, a bad slot or grid, a slot no finished
 * run covered.
 * ccd_dsens_passes: float-path passes one run spends on the slot, 2 * sum over its latent grids of min(S, h) * min(S, w)
 * (known at add).  ccd_dsens_destroy drains the streams the handle was given. */
typedef struct ccd_dsens ccd_dsens;
int ccd_latent_footprint(const ccd_cc_header* arch, int grid, int32_t box[4]);
int ccd_latent_probe_stride(const ccd_cc_header* arch, int grid, int frame_data_type);
int ccd_dsens_create(int device, int n_probe_slots, ccd_dsens** out);
void ccd_dsens_destroy(ccd_dsens* d);
int ccd_dsens_add(ccd_dsens* d, const ccd_cc_header* arch, const uint8_t* bytes_nn, size_t n_nn, const int8_t* const* latents,
                  const void* const* src, int bitdepth, int frame_data_type);
/* One cool-chic of a P / B frame as a candidate.  A P / B frame is decoded from two cool-chics, residue
 * and motion, whose synthesis outputs go through ccd_inter_reconstruct; the candidate is ONE of them (`role`), the other one's
 * output is given (`partner`) and held fixed.  Everything is as for ccd_dsens_add - layout, sentinels, hyperlatent zeros, maps
 * that do not depend on n_probe_slots or on what else the handle holds - and an entry is
 *
 *     dD[s][g][y][x] = SSE(reconstruct(output of this cool-chic with latent[g][y][x] + s, partner as given, references))
 *                    - SSE(reconstruct(output of this cool-chic as given, partner, references))
 *
 * where reconstruct is exactly ccd_inter_reconstruct.  The reconstruction is pointwise (sample (y, x) reads both outputs at (y, x)
 * only), so ccd_latent_footprint and ccd_latent_probe_stride hold for both cool-chics of the frame.  `arch`, `bytes_nn`, `latents`:
 * the candidate cool-chic; `src`, `bitdepth`, `frame_data_type` (0, 1, 2): the FRAME's; the frame's size is arch->img_size.
 * `partner`, the references and `src` are read at every run and never written; they must stay valid while the handle may run (a
 * caller that changed the partner's buffer between runs is followed, like latents changed in place).  The two cool-chics of a
 * frame are two independent slots; intra and inter candidates may share a handle.  ccd_dsens_passes counts as for ccd_dsens_add.
 * Per run the references are converted once, the base slots of all inter candidates are reconstructed by one launch (two when
 * both the sinc-8 and another filter size are in use) behind the first round's float path - it keeps the warped references of
 * residue candidates, which their probes only read - and every round reconstructs its probe slots by one such launch.
 * CCD_ERR_ARG - before the device is touched - for a NULL argument, `inter`, partner, ref0[p] or (B frames) ref1[p], a frame_type
 * outside 1..2, a role outside 0..1, a bit depth outside 8..16, a frame_data_type other than 0, 1, 2, a run in flight;
 * CCD_ERR_VALUE - also before the device is touched - for an `arch` that does not re-parse, a filter size ccd_inter_reconstruct
 * refuses, yuv420 with an odd side, an `arch` whose out_channels is not what the role needs (residue: 4 for P, 5 for B; motion:
 * 2 for P, 4 for B). */
typedef struct {
    int32_t frame_type;         /* 1 P, 2 B (as ccd_inter_reconstruct) */
    int32_t role;               /* 0: the candidate is the frame's residue cool-chic, 1: its motion cool-chic */
    const float* partner;       /* DEVICE f32 synthesis output of the OTHER cool-chic: role 0: motion [2|4][h][w]; role 1: residue [4|5][h][w] */
    const void* ref0[3];        /* DEVICE integer planes of the references, layout of ccd_inter_reconstruct */
    const void* ref1[3];        /* B frames */
    int32_t global_flow[4];
    int32_t warp_filter_size;   /* 2, 4, 6..16 even */
} ccd_dsens_inter;
int ccd_dsens_add_inter(ccd_dsens* d, const ccd_cc_header* arch, const uint8_t* bytes_nn, size_t n_nn, const int8_t* const* latents,
                        const void* const* src, int bitdepth, int frame_data_type, const ccd_dsens_inter* inter);
int ccd_dsens_run(ccd_dsens* d, void* stream);
int ccd_dsens_wait(ccd_dsens* d, void* stream);
int64_t ccd_dsens_slot_map(const ccd_dsens* d, int slot, int grid, void** dev_ptr);
int ccd_dsens_passes(const ccd_dsens* d, int slot);
/* Distortion deltas through the frames that predict from a moved one.  The planes of an I or P frame
 * are references of other frames: a DEPENDENT F of slot `slot` is a P / B frame whose reference number `which` is the frame R
 * that the slot decodes (intra, or one cool-chic of a P / B frame).  For every grid, position and sign
 *
 *     dDdep[s][g][y][x] = sum over the slot's dependents F of
 *         SSE_F(reconstruct(F's residue, F's motion, references with R := planes decoded with latent[g][y][x] + s))
 *       - SSE_F(reconstruct(F's residue, F's motion, references with R := planes as decoded))
 *
 * with reconstruct exactly ccd_inter_reconstruct and SSE_F the squared error of F's three integer planes against F's source.
 * F's two float outputs, its other reference (B frames), its source and its global flow are given and held fixed: read at every
 * run and never written, like `partner` (a caller that rewrote them between runs is followed).  F's size, bit depth and
 * frame_data_type are the candidate's.  Only DIRECT dependents count: frames that predict from F are not followed.
 * Layout int64 [2][h][w] per grid, INT64_MIN where v + s leaves [-64, 63], hyperlatent grids zeros with those sentinels: as the
 * own map, which ccd_dsens_slot_map keeps handing out unchanged in meaning and in value (the slot's own frame only).
 * The warp is not pointwise in the reference, so the change of one latent scatters into F where F's flows point.  A slot with
 * dependents plans its passes with a wider stride, ccd_latent_probe_stride_margin(arch, grid, frame_data_type, margin) with
 * margin = W - 1 (rgb, yuv444) or W + 2 (yuv420), W the widest window of its dependents' warps (2 bilinear, 4 bicubic, the filter
 * size for sinc), on every grid; ccd_dsens_passes reports the new count.  With that margin one window never reads the regions of
 * two latents of a pass, and a 4:2:0 quad does not either while the integer tap offsets of its four flows differ by at most 2
 * per axis.  Where a unit (a luma sample, or a 4:2:0 quad with its chroma sample) still reads two regions its change cannot be
 * split: the entries involved are CONFLICTS, INT64_MIN in the map like an illegal move, and ccd_dsens_slot_dep_conflicts counts
 * the legal ones per grid.  A slot without dependents keeps its strides, passes and maps to the bit.
 * ccd_dsens_add_dependent: CCD_ERR_ARG - before the device is touched - for a NULL argument (residue, motion, src[p] and, B frames,
 * other_ref[p] included), a bad slot, a frame_type outside 1..2, `which` outside 0..1 or 1 for a P frame, a run in flight;
 * CCD_ERR_VALUE for a filter size ccd_inter_reconstruct refuses, or a yuv420 candidate with an odd side.
 * ccd_dsens_slot_dep_map / ccd_dsens_slot_dep_conflicts: as ccd_dsens_slot_map; CCD_ERR_ARG also for a slot without dependents.
 * ccd_latent_probe_stride_margin (host only): ccd_latent_probe_stride with `margin` samples kept strictly between the regions
 * of two latents a stride apart (margin 0: ccd_latent_probe_stride); CCD_ERR_ARG also for a negative margin. */
typedef struct {
    int32_t frame_type;        /* 1 P, 2 B: the DEPENDENT's */
    int32_t which;             /* the candidate's frame is the dependent's reference 0 or 1 (P: 0) */
    const float* residue;      /* DEVICE f32 [4|5][h][w] */
    const float* motion;       /* DEVICE f32 [2|4][h][w] */
    const void* other_ref[3];  /* B frames: DEVICE planes of the reference that is not the candidate */
    const void* src[3];        /* DEVICE planes of the dependent's source */
    int32_t global_flow[4];
    int32_t warp_filter_size;
} ccd_dsens_dependent;
int ccd_dsens_add_dependent(ccd_dsens* d, int slot, const ccd_dsens_dependent* dep);
int64_t ccd_dsens_slot_dep_map(const ccd_dsens* d, int slot, int grid, void** dev_ptr);
int64_t ccd_dsens_slot_dep_conflicts(const ccd_dsens* d, int slot, int grid);
int ccd_latent_probe_stride_margin(const ccd_cc_header* arch, int grid, int frame_data_type, int margin);
/* Host only (tests): the lattice geometry of csrc/ccd_lattice.hpp on one axis given by its numbers: n latents over N samples,
 * the footprint interval [lo, hi] around floor(i num / den), `even` the 4:2:0 widening of the regions.  ccd_debug_lattice_stride:
 * the smallest stride that keeps `margin` samples between two regions (n when none does).  ccd_debug_lattice_hit: which member
 * of the lattice (S, phase) has its region under the samples [a, b]: -1 none, its index for exactly one, -2 for more than one;
 * *first and *count (may be NULL) the first member hit and how many.  CCD_ERR_ARG for numbers that describe no axis. */
int ccd_debug_lattice_stride(int n, int N, int lo, int hi, uint32_t num, uint32_t den, int even, int margin);
int ccd_debug_lattice_hit(int n, int N, int lo, int hi, uint32_t num, uint32_t den, int even, int S, int phase, int a, int b, int32_t* first,
                          int32_t* count);

/* ---- One RDOQ step: choose and apply +-1 moves that do not interact (ccd_rdoq.hip, ccd_rdoq_api.cpp) ----
 * From the two delta maps of every grid - the distortion deltas of ccd_dsens_slot_map and the rate deltas of
 * ccd_enc_slot_delta_map, or any maps of those shapes - a step picks on the device a set of moves whose deltas add, and applies
 * them to the caller's device latents in place.
 * Two moves are independent when neither a symbol of the rate model reads both latents (p itself, its spatial dependents and
 * the IFCE blocks of the finer grids: DESIGN.md 4.10 "Rate sensitivity") nor a sample of the planes is reached by both
 * (ccd_latent_footprint, 4:2:0 chroma included).  The step tests a superset of that relation: the INFLUENCE BOX of a latent is
 * the bounding rectangle, in luma samples, of its clipped footprint and of area(r) for every symbol r of its rate set, where
 * area(g, qy, qx) = rows floor((qy << level[g]) H / h0) .. ceil(min((qy + 1) << level[g], h0) H / h0) - 1 (columns alike; h0 x w0
 * is grid 0, level[g] the number of size changes between grid 0 and grid g), expressed in cells of ccd_rdoq_cell() x
 * ccd_rdoq_cell() luma samples.  Latents whose boxes share no cell are independent.
 * ccd_rdoq_influence_box (host only): cells = {top, left, bottom, right}, inclusive, of the latent (y, x) of `grid`.  CCD_ERR_ARG
 * for NULL, a bad grid or position or a frame_data_type other than 0, 1, 2; CCD_ERR_VALUE for an `arch` that does not re-parse.
 * ccd_rdoq_add: latents[g] = DEVICE int8 [grid_h[g]][grid_w[g]], READ AND WRITTEN by every step; returns the slot.  CCD_ERR_ARG -
 * before the handle or the device is looked at - for a NULL argument or a frame_data_type other than 0, 1, 2; for a step in flight.
 * ccd_rdoq_set_maps: dd[g] = device int64 [2][h][w] (plane 0: the change of the squared error for v - 1, plane 1 for v + 1;
 * INT64_MIN: no such move; a NULL dd[g] stands for zeros, as a hyperlatent grid's map is), dbits[g] = device float32 [2][h][w]
 * (a non-finite entry: no such move).  Read by every later step.
 * ccd_rdoq_step: per-slot arrays.  The cost of a move is c = dD * kD + dBits * kR in float64 (two products, one sum, each
 * rounded once); a latent's better move (-1 on a tie of the costs as float32) is a candidate when its grid's bit of grid_mask is
 * set, the latent as it is now plus the move stays in [-64, 63] and c < -min_gain.  Candidates are ordered by the key
 * (cost as float32, then slot-wide index first[g] + y w + x); a candidate is selected when it has the smallest key of all
 * candidates whose boxes share a cell with its own, and the candidate with the slot's smallest key always is.  Selected latents
 * are stored as v + s.  Negative or non-finite kD, kR, min_gain, NULL arrays, a slot without maps and a step in flight are
 * CCD_ERR_ARG.  The call only enqueues; ccd_rdoq_wait synchronises.  One step may be in flight per handle.  ccd_rdoq_destroy drains
 * the streams the handle was given.
 * ccd_rdoq_step_rounds: the same step in max_rounds rounds (1 .. ccd_rdoq_max_rounds() = 64, else CCD_ERR_ARG before the handle or
 * the device is looked at); ccd_rdoq_step is max_rounds = 1.  Every candidate starts OPEN and no cell is TAKEN.  In a round (a) an
 * open candidate whose box holds a taken cell becomes BLOCKED for good and claims nothing, (b) the other open candidates compete
 * as above, (c) the winners are SELECTED and applied, (d) the cells of their boxes become taken.  A candidate that lost a cell to
 * a candidate that then lost elsewhere competes again in the next round, so the selected set grows from round to round towards
 * the set a walk over the candidates in ascending key order would take (each candidate taken unless its box shares a cell with an
 * earlier taken one), and equals it once a round selects nothing.  Whatever max_rounds, the selected set is pairwise independent,
 * a function of the maps and max_rounds alone, and the result and the move map cover all rounds.
 * ccd_rdoq_slot_open: the candidates that took part in the LAST round of the last finished step and were not selected.  0: the
 * selected set is maximal - every candidate is selected or shares a cell with a selected one; > 0: another round might select
 * more.  CCD_ERR_ARG as ccd_rdoq_slot_result.
 * ccd_rdoq_link: `slot` joins the claim raster of `leader`; from then on the two slots are a GROUP and every later step lets
 * their candidates compete as one population (two cool-chics that decode into one frame: the residue and the motion cool-chic of
 * a P / B frame, whose reconstruction is pointwise).  The key of a group is (cost as float32, group-wide index): the leader's
 * latents keep first[g] + y w + x, the follower's get total(leader) + first[g] + y w + x, so the leader's candidate wins a tie of
 * the costs (a slot holds at most 2^31 - 1 latents: 32 bits hold both).  The rule of ccd_rdoq_step / ccd_rdoq_step_rounds holds
 * with "slot" read as "group": a candidate is selected when it has the smallest key of all candidates of the group whose boxes
 * share a cell with its own, the candidate with the group's smallest key always is, the cells taken in a round block the open
 * candidates of either slot in the later rounds, and the fixed point is the walk over the group's candidates in ascending key
 * order.  Costs, admission (kD, kR, min_gain, grid_mask), results, move maps and ccd_rdoq_slot_open stay per slot; a slot whose
 * grid_mask is 0 offers nothing, and its partner then steps as if it were not linked.  CCD_ERR_ARG before the handle is looked
 * at: a NULL r, a negative index, slot == leader; CCD_ERR_ARG also for an index past the slots, a step in flight, a slot or
 * leader that already belongs to a group (pairs only; a follower cannot lead); CCD_ERR_VALUE when the two slots differ in
 * frame_data_type or img_size (their rasters would not be congruent).  A refused link leaves the handle as it was.  Allowed
 * before the first step and between steps; there is no unlink.  Linked pairs and plain slots may share a handle, and a slot
 * nobody linked steps exactly as without this call.
 * ccd_rdoq_slot_result: what the last finished step did; d_bits is a float64 sum in an order that depends on the geometry only
 * (the same words on a second call), d_cost = kD * d_sse + kR * d_bits.  ccd_rdoq_slot_moves: device int8 [h][w], the step's
 * move (-1, 0, +1) at every latent, and h * w as the return value; valid until the next step / destroy.  Both CCD_ERR_ARG for a
 * NULL argument, a bad slot or grid, a slot no finished step covered. */
typedef struct ccd_rdoq ccd_rdoq;
typedef struct {
    int32_t status, n_grids;
    int64_t n_candidates, n_moves;
    int64_t n_moves_grid[CCD_MAX_GRIDS];
    int64_t d_sse;      /* exact: sum of the chosen dD */
    double d_bits;      /* sum of the chosen dBits */
    double d_cost;
} ccd_rdoq_result;
int ccd_rdoq_cell(void);
int ccd_rdoq_max_rounds(void);
int ccd_rdoq_influence_box(const ccd_cc_header* arch, int frame_data_type, int grid, int y, int x, int32_t cells[4]);
int ccd_rdoq_create(int device, ccd_rdoq** out);
void ccd_rdoq_destroy(ccd_rdoq* r);
int ccd_rdoq_add(ccd_rdoq* r, const ccd_cc_header* arch, int frame_data_type, int8_t* const* latents);
int ccd_rdoq_set_maps(ccd_rdoq* r, int slot, const int64_t* const* dd, const float* const* dbits);
int ccd_rdoq_link(ccd_rdoq* r, int slot, int leader);
int ccd_rdoq_step(ccd_rdoq* r, const double* kD, const double* kR, const double* min_gain, const uint64_t* grid_mask, void* stream);
int ccd_rdoq_step_rounds(ccd_rdoq* r, const double* kD, const double* kR, const double* min_gain, const uint64_t* grid_mask, int max_rounds,
                         void* stream);
int ccd_rdoq_wait(ccd_rdoq* r, void* stream);
int ccd_rdoq_slot_result(const ccd_rdoq* r, int slot, ccd_rdoq_result* out);
int64_t ccd_rdoq_slot_open(const ccd_rdoq* r, int slot);
int64_t ccd_rdoq_slot_moves(const ccd_rdoq* r, int slot, int grid, void** dev_ptr);

/* ---- Claims that follow the flows into the dependent frames ----
 * Slot `slot` decodes a frame R (intra, or either cool-chic of a P / B frame).  A FOLLOW names a dependent F, a P / B frame with R
 * as its reference `which`: F's device motion output (f32 [2 | 4][h][w], read at every step, never written), its global flow and
 * warp filter size, `target` - the slot of this handle in whose claim raster F's samples are claimed: F's residue slot, or the
 * leader of F's linked pair; a caller that holds F fixed still adds that slot and gives it grid_mask 0 - and `frozen`, the slot of
 * F's motion cool-chic in this handle, or -1.  R and F have one img_size and frame_data_type.
 * From the next step on a candidate of `slot` claims, beside its influence box, its FLOW BOX in the raster of every follow's
 * target: per step a REACH TABLE is built from the flows as they then are - for every cell C (ccd_rdoq_cell() luma samples a side)
 * of F the bounding rectangle of the reference indices the windows of its samples read (the index pieces of the warp), and for
 * every cell c of R that rectangle meets reach[c] = bbox(reach[c], C) - and the flow box of a latent is the bounding rectangle of
 * reach[c] over the cells c of its influence box, empty if all are.  A candidate is blocked when a cell of this CLAIM SET is taken,
 * claims in every cell of it and is selected when its key stands in all of them; the rule of ccd_rdoq_step_rounds holds with
 * "box" read as "claim set".  Slots connected by links or follows form a COMPONENT whose latents share one numbering (the groups
 * in ascending order of their leader's slot, the leader's latents before the follower's); a slot in no follow relation keeps its
 * numbering and steps exactly as without these calls.  Two selected moves change disjoint sets of samples of R and of every
 * followed F, so own and dependent deltas add.  Only DIRECT dependents: what predicts from F is not followed.
 * ccd_rdoq_follow returns the follow's index (0 .. ccd_rdoq_max_follows() - 1 = 3).  CCD_ERR_ARG before the handle is looked at: a
 * NULL r / f / motion, a negative slot or target, frozen < -1, frame_type outside 1 .. 2, which outside 0 .. frame_type - 1;
 * CCD_ERR_ARG also for an index past the slots, a step in flight, a fifth follow; CCD_ERR_VALUE for target == slot, a
 * warp_filter_size ccd_inter_reconstruct refuses, a target of another img_size or frame_data_type, and a component that would
 * hold 2^32 latents or more (ccd_rdoq_link refuses that too).  A refused call leaves the handle as it was.  There is no unfollow.
 * ccd_rdoq_set_dep_maps: dd_dep[g] = device int64 [2][h][w], the dependent map of ccd_dsens_slot_dep_map, or NULL; the cost
 * becomes (dD + dDdep) * kD + dBits * kR and a move exists in neither map's INT64_MIN.  dd_dep == NULL, or all entries NULL:
 * the rule of ccd_rdoq_step to the bit.  ccd_rdoq_result.d_sse stays the change of the slot's OWN frame;
 * ccd_rdoq_slot_dep_sse gives the exact sum of the chosen dependent entries, and d_cost = kD * (d_sse + dep_sse) + kR * d_bits.
 * ccd_rdoq_step / ccd_rdoq_step_rounds return CCD_ERR_VALUE, before anything is enqueued, when the `frozen` slot of any follow
 * has a non-zero grid_mask: the flows are followed as given, and no map prices a flow that moves in the same step.
 * ccd_rdoq_slot_reach: the reach table of the last finished step, device uint32 [cells_h][cells_w][4] =
 * {top, left, ~bottom, ~right} in cells of F (all ones: no sample of F reads the cell); returns cells_h * cells_w.
 * ccd_rdoq_slot_flow_boxes: device uint16 [h][w][4] = {top, left, bottom, right} of every latent of `grid`, top > bottom: empty;
 * returns h * w.  Both valid until the next step / destroy; CCD_ERR_ARG as ccd_rdoq_slot_moves, and for a follow no finished
 * step covered. */
typedef struct {
    int32_t frame_type;        /* of F: 1 P, 2 B */
    int32_t which;             /* F's reference that `slot` decodes */
    const float* motion;       /* DEVICE f32 [2 | 4][h][w]: F's motion output */
    int32_t global_flow[4];    /* F's, as ccd_inter_reconstruct takes it */
    int32_t warp_filter_size;
    int32_t target;            /* the slot whose raster F's samples are claimed in */
    int32_t frozen;            /* the slot of F's motion cool-chic, or -1 */
} ccd_rdoq_follow_desc;
int ccd_rdoq_max_follows(void);
int ccd_rdoq_lane_cells(void);  /* a box or flow box of more cells than this is walked by a wave, not a lane (a cost figure, not a limit) */
int ccd_rdoq_follow(ccd_rdoq* r, int slot, const ccd_rdoq_follow_desc* f);
int ccd_rdoq_set_dep_maps(ccd_rdoq* r, int slot, const int64_t* const* dd_dep);
int ccd_rdoq_slot_dep_sse(const ccd_rdoq* r, int slot, int64_t* out);
int64_t ccd_rdoq_slot_reach(const ccd_rdoq* r, int slot, int follow, void** dev_ptr);
int64_t ccd_rdoq_slot_flow_boxes(const ccd_rdoq* r, int slot, int follow, int grid, void** dev_ptr);

/* ---- the squared error of many candidates of P / B frames per launch ----
 * A FRAME is a P / B frame as ccd_inter_reconstruct takes it - the f32 outputs of its residue and motion cool-chics (its base
 * pair), the integer planes of its references, global flow, filter size - and the planes of its source.  An ITEM is that frame
 * with the output of ONE of the two cool-chics replaced: role 0 another residue output [4 | 5][h][w], role 1 another motion
 * output [2 | 4][h][w].  For the base pair of every frame and for every item a run gives, per plane,
 *
 *     sse[p] = sum over the plane of (ccd_inter_reconstruct(residue, motion, references)[p] - src[p])^2
 *
 * as exact integers - what ccd_inter_reconstruct followed by ccd_quality_score_batch reports, from the same device functions -
 * and n[p], the plane's sample count.  No plane is stored.  All pointers are DEVICE pointers, read at every run and never written;
 * they must stay valid while the handle may run (a caller that rewrote a buffer between runs is followed, as with `partner` of
 * ccd_dsens_add_inter).  frame_data_type 0 rgb, 1 yuv420, 2 yuv444; planes u8 at 8 bits, else u16.
 * Per run: the references of every frame are converted once, the base pairs of all frames are scored by one launch (which keeps
 * their warped references: a residue item only reads those), all items by one more (each of the two becomes two launches when
 * both the sinc-8 and another filter size are present), and one small launch adds up the workgroup partials.  A result does
 * not depend on what else the handle holds.  ccd_iscore_run only enqueues on `stream`; ccd_iscore_wait synchronises.  One run
 * may be in flight per handle.  ccd_iscore_clear_items drops the items and keeps the frames (a long list is priced in chunks);
 * ccd_iscore_destroy drains the streams the handle was given.  Scratch comes from the block cache: ccd_iscore_add_frame takes
 * the frame's (references and warped references as 4:4:4 f32), ccd_iscore_run the tables and partials; CCD_ERR_NOMEM from either.
 * ccd_iscore_add_frame / ccd_iscore_add return the frame / item index.  ccd_iscore_frame_result / ccd_iscore_result: sse[3] and
 * n[3] of a base pair / an item the last finished run covered.
 * CCD_ERR_ARG - before the device is touched - for a NULL argument (residue, motion, ref0[p], src[p] and, B frames, ref1[p]
 * included), a frame_type outside 1..2, a role outside 0..1, a bit depth outside 8..16, a frame_data_type outside 0..2, a frame or
 * item index out of range (or not covered by a finished run), a run in flight; CCD_ERR_VALUE - also before the device is touched -
 * for a filter size ccd_inter_reconstruct refuses, yuv420 with an odd side, a side outside 1..16383.  A refused call leaves the
 * handle as it was.
 *
 * REFERENCE ITEMS: ccd_iscore_add_refs adds the frame's BASE pair reconstructed against OTHER integer
 * planes in place of reference 0 (ref0), reference 1 (ref1, B frames) or both - the planes a candidate of the REFERENCE frame
 * decodes to - in the layout of ccd_inter_reconstruct (u8 at 8 bits, else u16; half-size chroma for yuv420).  A NULL array means
 * "the frame's own reference".  It returns the item index in the SAME index space as ccd_iscore_add; the result comes from
 * ccd_iscore_result, ccd_iscore_clear_items drops these items too.  The planes are read at every run and never written.
 * Scratch: ccd_iscore_add_refs takes 3 h w f32 per replaced reference from the block cache (CCD_ERR_NOMEM otherwise),
 * ccd_iscore_clear_items and ccd_iscore_destroy give it back.
 * Launches of a run, in order: the references of the frames (one conversion per reference); the base pairs; the conversion of
 * the replaced references of ALL reference items (one launch over a job table); the items, role and reference items together
 * (two launches where sinc-8 and another filter size are both present, as for the base pairs); the final sum.  A reference item
 * of a B frame with one reference replaced warps only that one and reads the other's warp as the base pair of the same run kept
 * it; no item writes the kept warps.  A result does not depend on what else the handle holds.
 * CCD_ERR_ARG - before the device is touched - for a NULL handle, a frame index out of range, both arrays NULL, an array with a
 * NULL plane in it, ref1 given for a P frame, a run in flight.  A refused call leaves the handle as it was. */
typedef struct ccd_iscore ccd_iscore;
typedef struct {
    int32_t frame_type;        /* 1 P, 2 B */
    int32_t h, w, bitdepth, frame_data_type;
    const float* residue;      /* DEVICE f32 [4 | 5][h][w]: the base pair */
    const float* motion;       /* DEVICE f32 [2 | 4][h][w] */
    const void* ref0[3];       /* DEVICE integer planes of the references, layout of ccd_inter_reconstruct */
    const void* ref1[3];       /* B frames */
    const void* src[3];        /* DEVICE planes of the frame's source */
    int32_t global_flow[4];
    int32_t warp_filter_size;  /* 2, 4, 6..16 even */
} ccd_iscore_frame;
int ccd_iscore_create(int device, ccd_iscore** out);
void ccd_iscore_destroy(ccd_iscore* s);
int ccd_iscore_add_frame(ccd_iscore* s, const ccd_iscore_frame* frame);
int ccd_iscore_add(ccd_iscore* s, int frame, int role, const float* output);
int ccd_iscore_add_refs(ccd_iscore* s, int frame, const void* const ref0[3], const void* const ref1[3]);
int ccd_iscore_clear_items(ccd_iscore* s);
int ccd_iscore_run(ccd_iscore* s, void* stream);
int ccd_iscore_wait(ccd_iscore* s, void* stream);
int ccd_iscore_frame_result(const ccd_iscore* s, int frame, uint64_t* sse, uint64_t* n);
int ccd_iscore_result(const ccd_iscore* s, int item, uint64_t* sse, uint64_t* n);

/* Leaky-quantised-Laplace boundaries computed ON THE GPU for a list of (mu_idx, scale_idx, s):
 * left[i], right[i] as the entropy kernel sees them (exhaustive parity tests of the f64 CDF). */
int ccd_debug_laplace_bounds(int device, const int32_t* mu_idx, const int32_t* scale_idx, const int32_t* s,
                             int64_t n, uint32_t* left, uint32_t* right);

/* Exhaustive form of the above (tools/cdf_sweep.py): the left cumulative of EVERY symbol s = -63 .. 63 for EVERY mu index and
 * the scale indices [scale_first, scale_first + n_scales), computed on the GPU by the production kernel's table builder
 * (which = 0: window_left, ccd_entropy_pipe.hip) or the generic kernel's (which = 1: laplace_left, ccd_entropy.hip).
 * out (host) receives n_scales * 32768 * 127 words, [scale][mu_idx][s + 63]. */
int ccd_debug_laplace_sweep(int device, int which, int scale_first, int n_scales, uint32_t* out);

/* Host only: 1 when this cool-chic's ARM runs on the pipelined entropy kernel: every ARM / stabiliser weight fits int32, no
 * hidden activation can leave int32 even for worst-case inputs, the worst-case IFCE feature fits the kernel's int32 side
 * plane (< 2^30), <= 32 ARM inputs, <= 8 layers, picture not wider than the symbol ring (5 060).  What depends on the data -
 * IFCE features as 16-bit operands - is checked per task on the device and the pixel redone in plain int64 (no trained
 * network takes it; tests/test_arm_envelope.py does).  0 when it needs the generic 64-bit kernel (~7x slower; no network the reference encoder produced
 * does), < 0 on a malformed header / payload. */
int ccd_network_fits_fast_path(const uint8_t* cc_header, size_t n_hdr, const uint8_t* bytes_nn, size_t n_nn);
/* Host only: WHICH entropy-kernel instantiation a batch with default options gives this cool-chic (tests and DESIGN.md's
 * instantiation table): bit 0 = pipelined kernel (else the generic one), bit 4 = its instantiation with the device check of the
 * IFCE features (worst-case feature >= 2^15), bit 7 = the network is outside the finite envelope of the float stages (vector-ALU
 * float kernels only), bits 8..11 = NV = ceil(ARM inputs / 4), bits 12..15 = ARM layers (hidden + output).
 * Same bits 0, 4 and 7 as ccd_batch_slot_kernels.  Above them the decisions behind the choice, one bit each (the network's own
 * flags, whatever bit 0 says): bit 16 = `narrow` (32-bit operands and accumulators below 2^62 guaranteed: the generic kernel's
 * 32-bit form, and a condition of the matrix cores), bit 17 = every IFCE weight fits int32 (the register-resident feature
 * pass), bit 18 = a batch with CCD_OPT_MFMA_ARM = 1 runs this ARM on the matrix cores (ccd_batch_slot_kernels bit 3), bit 19 =
 * every ARM / stabiliser weight fits int32, bit 20 = a hidden activation could leave int32, bit 21 = the worst-case IFCE
 * feature is below 2^30, bit 22 = it is 2^15 or more (bit 4 without the "pipelined" condition).
 * < 0 on a malformed header / payload. */
int ccd_network_kernel_class(const uint8_t* cc_header, size_t n_hdr, const uint8_t* bytes_nn, size_t n_nn);

/* Profile builds only (-DCCD_FD_PROFILE): cycles per phase of the fused float kernel, summed over wave 0 of every
 * workgroup since the last reset; returns 1 with out16 filled, 0 when the library was built without the counters. */
int ccd_debug_fd_profile(uint64_t* out16, int reset);

#ifdef __cplusplus
}
#endif
#endif
