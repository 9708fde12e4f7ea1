// ccd_device.hpp - structures shared between the host API and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ccd.h"
#include "ccd_lattice.hpp"
#include "ccd_ratedelta_plan.hpp"

namespace ccd {

constexpr int kMaxCtx = 40;          // spatial context template size (arm.py:501-509)
constexpr int kAcLo = -64;           // symbols live in [-64, 63] (constants.py:11)
constexpr int kAlphabet = 128;
constexpr int kRcPrecision = 24;     // constriction default range-coder precision
constexpr int kMuOffset = 16384;     // -MU_MIN_FIXED_POINT (constants.py:31)
constexpr int kScaleOffset = 1280;   // -LOG_SCALE_MIN_FIXED_POINT (constants.py:36)
constexpr int kNumMu = 32768, kNumScale = 2561;

// Which entry owns work item i of a launch over n entries (ingest segments, passes, planes, grids): the entry s with
// prefix[s] <= i < prefix[s + 1] (entries without work have prefix[s] == prefix[s + 1]).
__device__ __forceinline__ int entry_of(const uint32_t* prefix, int n, uint32_t i) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (prefix[mid + 1] <= i) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Per-slot description of the entropy stage (device memory, read-only for the kernel).
struct EntropyParams {
    const uint32_t* words;   // latent payload as little-endian u32 words
    uint32_t n_words;
    int32_t n_grids;
    int32_t grid_h[CCD_MAX_GRIDS], grid_w[CCD_MAX_GRIDS];
    int8_t* latent[CCD_MAX_GRIDS];     // decoded grids [h][w]
    int32_t ifce_in[CCD_MAX_GRIDS];    // number of IFCE input channels of the grid (0 = none)
    int32_t ifce_off[CCD_MAX_GRIDS];   // offset (in int64) of the grid's IFCE parameters in `ifce`
    int32_t level[CCD_MAX_GRIDS];      // number of size changes between grid 0 and grid g
    int32_t dim, n_spatial, n_ifce_out, n_layers, narrow, has_ifce;
    int32_t ctx_dy[kMaxCtx], ctx_dx[kMaxCtx];
    const int64_t* arm;      // per layer: w[in][out], b[out]; then ws[dim][2], bs[2]
    int32_t arm_len;         // length of `arm` in int64
    const int64_t* ifce;     // per grid with IFCE: w[in][out], b[out]
    int32_t* ifce_feat;      // scratch [n_ifce_out][fh][fw] (features at the previous grid's size)
    const float* scale_table;  // 2561 float32 scales
    const double* rcp_table;   // RN(1 / (double)scale): correctly rounded reciprocals for the f64 quotient
    int32_t* status;         // [0] error code, [1] words consumed, [2..3] symbols decoded (lo, hi)
    int32_t ring_rows;       // rows of the decoded-symbol ring in LDS: power of two >= widest grid / 10 + 6
    // Pipelined kernel, dynamic operand check (ccd_entropy_pipe.hip, "exactness"): features are kept as int16 planes in
    // `ifce_feat`; a feature with |f| >= 2^feat_bits is stored as the sentinel -32768 there and in full in `ifce_wide`
    // (int32 planes of the same shape); a pixel that meets a sentinel is redone in plain int64.  15 in production; tests
    // lower it (8..14) to force the redo path on ordinary streams.
    int32_t* ifce_wide;
    int32_t feat_bits;
    int32_t ifce_w32;        // every IFCE weight fits int32: the register-resident feature pass may be used
    int32_t mfma;            // > 0: the ARM's layers run on the matrix cores (limb-split int8, ccd_entropy_pipe.hip); the value
                             // is the number of bits a hidden activation may have before the task is redone in int64 (23)
};

// Per-slot description of the device WRITER (ccd_encode.hip): the entropy model in the layout the decoder uses (`ep`: geometry,
// integer networks, Laplace tables; ep.latent are the grids to ENCODE, read-only; ep.words / ifce_feat / ring fields unused) plus
// where a pixel's interval goes.  Coding order: grids n-1 .. 0; inside a grid raster when W <= 9, else wavefront steps
// c = x + 10 y with the pixels of a step in increasing y (latent.py:66-140).
struct alignas(8) EncodePair { uint32_t left, width; };  // one 8-byte access
struct EncodeParams {
    EntropyParams ep;
    uint32_t n_symbols;
    uint32_t n_blocks;                           // workgroups of the contexts kernel: sum of ceil(H * W / 64) over the grids
    uint32_t block_first[CCD_MAX_GRIDS];         // first workgroup of grid g (grows with g)
    uint32_t grid_first[CCD_MAX_GRIDS];          // coding-order index of the first symbol of grid g
    const uint32_t* step_prefix[CCD_MAX_GRIDS];  // [W + 10 (H - 1)]: symbols of grid g coded before step c (null when W <= 9)
    EncodePair* pairs;                           // [n_symbols] (left, right - left), coding order
    uint32_t* out;                               // payload words
    uint32_t cap_words;                          // ccd_enc_payload_bound(n_symbols) / 4
};

// The rate meter of the device writer (encode_rate_kernel / encode_rate_final_kernel, DESIGN.md 4.10 "rate meter"): what a slot
// of a measure writes, next to the EncodeParams of the same index.  A symbol with the interval (left, width) costs
// 24 - log2(width) bits; sum_width is the exact integer checksum of the intervals.
struct RatePartial { double bits; uint64_t sum_width; };                  // one per workgroup of the rate kernel
struct RateGrid { double bits; uint64_t sum_width; int64_t n_symbols; };  // one per grid
struct RateParams {
    RatePartial* partial;         // [n_blocks], indexed like the rate kernel's blockIdx.x
    RateGrid* grids;              // [n_grids], followed by one double: the sum of bits over the grids 0 .. n_grids - 1
    float* map[CCD_MAX_GRIDS];    // per grid [h][w] bits of every latent, raster; null without a map
    int32_t* status;              // [0] error code of the slot
};

// Rate sensitivity (encode_delta_ifce_kernel / encode_delta_kernel, DESIGN.md 4.10 "Rate sensitivity"): what a slot of a
// measure_deltas writes.  The IFCE stage works on 8 x 8 tiles of every fine grid g that has coarser sources (ifce_in[g] > 0,
// g != n_grids - 1).  Source channel c of such a grid is grid g + 1 + c, sh = level[g + 1 + c] - level[g + 1]; one latent of it
// is read by an aligned square of side 2^(sh + 1) of grid g.  The stage leaves one float64 cell per aligned square of side
// 2^s, s = delta_cell_shift(sh) (a whole dependent block, or an 8 x 8 piece of one), per sign: plane (g, c) is
// [2][ceil(H / 2^s)][ceil(W / 2^s)], the planes of a grid follow each other from part_first[g].
constexpr int kDeltaTile = 8, kDeltaTileLog = 3;
constexpr int delta_cell_shift(int sh) { return sh + 1 < kDeltaTileLog ? sh + 1 : kDeltaTileLog; }
constexpr uint32_t delta_cells(int h, int w, int s) {  // one sign of one plane
    return static_cast<uint32_t>((h + (1 << s) - 1) >> s) * static_cast<uint32_t>((w + (1 << s) - 1) >> s);
}
struct DeltaParams {
    double* partial;                      // the IFCE stage's cells
    uint32_t part_first[CCD_MAX_GRIDS];   // first cell of fine grid g
    uint32_t tile_first[CCD_MAX_GRIDS];   // first workgroup of the IFCE stage that belongs to grid g (grows with g)
    uint32_t n_tiles;
    float* map[CCD_MAX_GRIDS];            // per grid [2][h][w]: plane 0 the change for v - 1, plane 1 for v + 1
};

// Rate-network parameter deltas (encode_rate_delta_kernel / encode_rate_delta_final_kernel): what a slot of a
// measure_param_deltas (the ARM's integers) or a measure_ifce_deltas (the IFCE's, 4.21) writes.  Row
// r = 2 (k - first) + (sign > 0) of the slot's table.  A wave walks chunk j of the slot's workgroups -
// [j kArmDeltaChunkBlocks, (j + 1) kArmDeltaChunkBlocks) of the rate kernel's numbering - for a tile of kArmDeltaTile candidates and
// leaves one cell per candidate; the final kernel adds a candidate's cells in chunk order.
// ARM: candidate c is row c, row == nullptr.  IFCE: the candidates are sorted by their grid (stably: a grid's weights, then its
// biases, each in stream order), so that a tile walks the blocks of as few grids as the count allows; row[c] is the row sorted
// candidate c answers.
struct ParamDeltaCell { double bits; int64_t sum_width, moved; };
struct RateDeltaParams {
    const RateDeltaMove* cand;  // [n_cand]
    const uint32_t* row;        // [n_cand], or nullptr: candidate c answers row c
    ParamDeltaCell* partial;    // [n_chunks][n_cand], indexed like cand
    ParamDeltaCell* out;        // [n_cand], indexed by row: +inf, 0, 0 for a candidate that is not legal
    uint32_t n_cand, n_chunks;
    int32_t path, pad;          // kArmDeltaGeneric / kArmDeltaIncremental: which instantiation prices the slot
};
// whose integers a table prices (the kernel's kKind) and whose entry a RateDeltaMove moves (encode_pixel_model's kMove: or none's)
enum { kRateDeltaNone = -1, kRateDeltaArm = 0, kRateDeltaIfce = 1 };

// One copy of the ingest launch (ccd_ingest.hip): latent grid `src` of a slot whose latents were GIVEN as device pointers
// (ccd_batch_add_latents) goes to `dst`, where the entropy kernel would have left it.  The segments of one slot are adjacent.
struct IngestSeg {
    const int8_t* src;
    int8_t* dst;
    uint32_t n;       // bytes = grid_h * grid_w
    int32_t slot;     // its status words are [64 slot, 64 slot + 64) of the batch's status array
};
constexpr uint32_t kIngestChunk = 4096;  // bytes one 64-lane workgroup of the ingest launch copies
constexpr int kIngestWordB = 4;          // the second of the two status words a given slot alternates between (ccd_ingest.hip)

// ---- distortion deltas (ccd_dsens.hip, ccd_dsens_api.cpp) ----
// One grid of one probe slot's private latent copy, written by dsens_apply_kernel: the caller's grid `src` goes to `dst`, and the
// latents on the lattice (y % stride == py, x % stride == px) go there as v + move where that stays inside [-64, 63].
// move == 0: a plain copy (the grid the slot probed in the round before, or every grid at the head of a run).
struct DsensSeg {
    const int8_t* src;
    int8_t* dst;
    uint32_t n;            // bytes = h * w
    int32_t w;
    int32_t stride, py, px;
    int32_t move;          // -1, 0, +1
};
// One pass as dsens_sse_kernel sees it: the probes (py + i stride, px + j stride), i < ny, j < nx, of a grid, the planes they
// were decoded to and where their entries go.  The box of the probe (y, x) is, in luma samples,
//   rows [(y * num_y) / den_y + box[0], (y * num_y) / den_y + box[2]], columns [(x * num_x) / den_x + box[1], .. + box[3]]
// clipped to the picture (ccd_latent_footprint); the 4:2:0 chroma planes take it halved, rounded outwards.  A probe's box is
// cut into `upp` bands of `rows` rows; a workgroup sums one band over the three planes into the round's slab.  ny == h, nx == w,
// stride == 1 and empty == 1 describe a hyperlatent grid: no samples, zeros and sentinels only.
struct DsensPass {
    const int8_t* lat;       // the caller's grid [h][w]: where v + move leaves the alphabet the entry is INT64_MIN
    int64_t* map;            // [2][h][w] of the grid
    const void* base[3];     // planes decoded from the latents as given
    const void* probe[3];    // planes of the probe slot that ran this pass
    const void* src[3];      // source planes
    int32_t h, w;            // of the grid
    int32_t stride, py, px, ny, nx;
    int32_t move;            // -1 / +1
    int32_t box[4];          // top, left, bottom, right
    uint32_t num_y, den_y, num_x, den_x;
    int32_t H, W;            // luma size
    int32_t chroma_shift;    // 1 for yuv420
    int32_t wide;            // samples are u16
    int32_t upp, rows;       // bands per probe, luma rows per band
    int32_t empty;
};
// ---- P / B frames reconstructed by units (ccd_inter.hip: dsens_inter_kernel, dsens_dep_kernel, inter_score_kernel; DESIGN.md
// 4.15, 4.16, 4.19; filled on the host by ccd_inter_job.hpp) ----
// One frame as the unit walk (di_unit) reconstructs it: the float outputs of the frame's two cool-chics go through the
// reconstruction of inter_recon_kernel and the integer step of planes_kernel.  A workgroup is a tile of 64 x 4 units, a unit one
// luma sample or, 4:2:0, one 2 x 2 luma quad and its chroma sample; the jobs of a launch share a prefix table of workgroups.
// What becomes of a quantised sample is the kernel's: dsens_inter_kernel stores it to `plane`, the other two compare it with a source.
struct InterUnitJob {
    const float* residue;    // [4 | 5][H][W]
    const float* motion;     // [2 | 4][H][W]
    const float* ref0;       // [3][H][W] f32, launch_planes_to_444 of the reference's planes
    const float* ref1;       // B frames
    float* w0;               // [3][H][W] the warped reference: written by mode 0 (null: not kept), read by mode 1 (and 4)
    float* w1;               // B frames (read by mode 1 and 3)
    void* plane[3];          // u8 / u16 planes: written by dsens_inter_kernel, the base read by dsens_dep_kernel, else null
    int32_t mode;            // 0 base: warp and keep, 1 residue probe: the kept warps, 2 motion probe: warp; B frames with one
                             // reference replaced: 3 warp ref0 and read w1, 4 read w0 and warp ref1.  Only mode 0 writes w0 / w1.
    int32_t frame_type, H, W, n_taps;
    int32_t gflow[4];
    int32_t chroma_shift;    // 1 for yuv420
    int32_t wide;            // samples are u16
    int32_t tiles_x;         // workgroups per row of workgroups
    float maxv;              // 2^bitdepth - 1
};
static_assert(sizeof(InterUnitJob) == 128, "InterUnitJob is a table entry: host and device agree on its layout");
// One (candidate, dependent, probe slot) of a round as dsens_dep_kernel sees it.  `recon` is the DEPENDENT frame
// (an InterUnitJob, mode 2) with the candidate's probe planes, as f32, in place of reference `which`; recon.plane are the
// dependent's BASE planes, which are only read here.  A unit whose windows into the reference touch the region of exactly one
// member of the pass's lattice adds its squared-error change to that entry of `acc`; one that touches several sets their bytes
// of `flag`.
struct DsensDepJob {
    InterUnitJob recon;
    const void* src[3];        // the dependent's source planes
    unsigned long long* acc;   // [2][h][w] of the grid: the dependent map while it is summed (two's complement)
    uint8_t* flag;             // [2][h][w]: 1 = a unit saw this entry together with another
    int32_t which;             // the reference of the dependent that is the candidate's frame
    int32_t h, w;              // of the grid
    int32_t move;              // -1 / +1
    int32_t stride, py, px;    // the pass's lattice
    LatticeAxis ay, ax;        // rows, columns
};
// One candidate of one P / B frame as inter_score_kernel sees it.  `recon` is the frame (an InterUnitJob; mode 0:
// the frame's base pair, 1: another residue output, 2: another motion output) - its planes are never stored, recon.plane stays
// null: the squared error of every sample against `src` is summed instead, per plane, one partial per workgroup.
struct InterScoreJob {
    InterUnitJob recon;
    const void* src[3];        // the frame's source planes
    uint32_t part_first;       // workgroup k of the job owns the partials [3 (part_first + k), 3 (part_first + k) + 3)
    uint32_t pad;
};
// One frame's integer planes -> the [3][h][w] f32 tensor the warp reads, as a job of planes_to_444_jobs_kernel (a replaced
// reference of a reference item): workgroups are 64 x 4 tiles of pixels, tiles_x per row.
struct PlanesConvJob {
    const void* p[3];          // u8 / u16 planes, chroma half-size where chroma_half
    float* out;
    int32_t h, w, chroma_half, wide;
    int32_t tiles_x;
    float maxv;                // 2^bitdepth - 1
};
static_assert(sizeof(PlanesConvJob) == 56, "PlanesConvJob is a table entry: host and device agree on its layout");
// The partials of one job as inter_score_final_kernel sums them: workgroups [first, first + count) of the partial array.
struct InterScoreRange { uint32_t first, count; };
// the frame of a job of any of the three kernels
__host__ __device__ inline const InterUnitJob& unit_job(const InterUnitJob& J) { return J; }
__host__ __device__ inline const InterUnitJob& unit_job(const DsensDepJob& D) { return D.recon; }
__host__ __device__ inline const InterUnitJob& unit_job(const InterScoreJob& S) { return S.recon; }
// One grid of a candidate with dependents as dsens_dep_final_kernel sees it (ccd_dsens.hip): entry e of [2][h][w] becomes INT64_MIN
// where the move leaves the alphabet or the entry is flagged, and the flagged legal entries are counted.
struct DsensDepGrid {
    const int8_t* lat;
    int64_t* map;
    const uint8_t* flag;
    unsigned long long* conflicts;
    uint32_t n;                // h * w
};
constexpr uint32_t kDsensChunk = 4096;   // bytes one 64-lane workgroup of dsens_apply_kernel writes
constexpr int kDsensBandSamples = 4096;  // luma samples of a band, about

// ---- RDOQ step (ccd_rdoq.hip, ccd_rdoq_api.cpp) ----
constexpr int kRdoqCell = 8;             // luma samples per side of a claim-raster cell (even: a 4:2:0 chroma sample lies in one cell)
constexpr uint32_t kRdoqLaneCells = 32;  // a box of up to this many cells is walked by its latent's lane, a larger one by a wave
constexpr uint32_t kRdoqChunk = 1024;    // latents one workgroup of the reduce launch sums
constexpr int kRdoqMaxRounds = 64;       // rounds of one step at most (ccd_rdoq_max_rounds)
constexpr uint8_t kRdoqSelected = 4, kRdoqBlocked = 8;  // bits of a pick byte beside the candidate's 1 / 2
// The influence box of a latent in cells of the claim raster, inclusive (ccd_rdoq_influence_box).
struct RdoqBox { uint16_t top, left, bottom, right; };
// One grid of one slot.  The latents of a slot are numbered uid = first + y * w + x over its grids; those of a linked pair
// (ccd_rdoq_link) over the leader's grids, then the follower's.
struct RdoqGrid {
    int8_t* lat;             // the caller's grid [h][w]: the only memory of the caller's a step writes
    const int64_t* dd;       // [2][h][w], nullptr: zeros
    const float* db;         // [2][h][w]
    int8_t* moves;           // [h][w]: -1, 0, +1
    uint8_t* pick;           // [h][w]: 0 no candidate, 1 candidate for -1, 2 candidate for +1 (claim -> select, reduce), with
                             // kRdoqSelected / kRdoqBlocked once a round has settled the candidate; neither: open
    const RdoqBox* box;      // [h][w]
    const uint32_t* big;     // indices y * w + x of the latents whose box has more than kRdoqLaneCells cells, ascending
    uint32_t n, first;       // h * w; uid of (0, 0)
    int32_t slot, grid;
};
struct RdoqSlot {
    unsigned long long* raster;  // [cells_h][cells_w] claim words, all ones between two rounds and between two steps
    uint8_t* taken;              // [cells_h][cells_w]: 1 for a cell of a box selected in an earlier round of this step, 0 between steps
    int32_t cells_h, cells_w;
    double kD, kR, min_gain;
    uint64_t grid_mask;          // bit g admits the candidates of grid g
    int32_t first_grid, n_grids; // its entries of the grid table
    uint32_t raster_units;       // 16-byte units of the raster block
    uint32_t taken_units;        // ... and of the taken block
    int32_t partner;             // the other slot of its pair (ccd_rdoq_link), -1: none
    int32_t owns_raster;         // 0 for a follower: raster and taken are its leader's, which settles and resets them
};
// What one workgroup of the reduce launch leaves for a chunk of kRdoqChunk latents of one grid.
struct RdoqPartial { int64_t n_candidates, n_moves, d_sse; double d_bits; int64_t n_open; };

// ---- claims that follow the flows into the dependent frames (ccd_rdoq_follow).  Everything a following step
// needs beyond RdoqGrid / RdoqSlot sits in tables of its own, entry for entry beside those, so that the kernels of a handle
// without follows read what they always read.
constexpr int kRdoqMaxFollows = 4;       // follows of one slot at most (ccd_rdoq_max_follows)
// A reach table: per cell c of the followed slot's raster four words, all of them minima over the cells C = (Y, X) of the
// dependent whose samples can read c: {min Y, min X, ~max Y, ~max X}.  All ones: nobody reads c.  One memset resets it.
constexpr int kRdoqReachWords = 4;
// One follow as rdoq_reach_kernel (ccd_inter.hip) sees it: the dependent F's flows into its reference `which`.
struct RdoqReachJob {
    const float* motion;     // F's motion output [2 | 4][H][W], read at every step
    uint32_t* reach;         // [cells_h][cells_w][kRdoqReachWords]
    int32_t which, H, W, n_taps;
    int32_t gx, gy;          // F's global flow for reference `which`
    int32_t cells_h, cells_w;
};
struct RdoqFollowRef {
    const uint32_t* reach;       // the follow's reach table
    unsigned long long* raster;  // the rasters of the follow's target (its group's)
    uint8_t* taken;
};
struct RdoqSlotX {
    int32_t n_follows;
    int32_t comp_first, comp_n;  // the slot's component: its entries of the tables of first uids / slots, uids ascending
    int32_t pad;
    RdoqFollowRef follow[kRdoqMaxFollows];
};
struct RdoqGridX {
    const int64_t* dd_dep;              // [2][h][w] the dependent map (ccd_rdoq_set_dep_maps), nullptr: none
    RdoqBox* fbox[kRdoqMaxFollows];     // [h][w] per follow: the flow box of every latent; top > bottom: empty
};
// What the reduce launch writes (a kernel argument, by value: it is only stored through).
struct RdoqSums {
    RdoqPartial* partial;          // [n_chunks]
    ccd_rdoq_result* results;      // [n_slots]
    int64_t* open;                 // [n_slots] candidates still open after the last round
    int64_t* partial_dep;          // [n_chunks], [n_slots]: the dependent maps' sums, with RdoqStepTables::gx only
    int64_t* dep_out;
};

// Upsampling level: stack_in [c_in][h_in][w_in] f32 (or the coarsest int8 grid) ->
// stack_out [c_in + 1][h_out][w_out]; channel 0 = pre-concat conv of the int8 grid `target`.
struct UpsampleLevel {
    const float* in_f32;     // nullptr when the input is the coarsest latent itself
    const int8_t* in_i8;
    const int8_t* target;    // [h_out][w_out]
    float* out;
    int32_t c_in, h_in, w_in, h_out, w_out;
    int32_t ups_k, pre_k;
    float ups_w[16], pre_w[16];
};

// Fused synthesis (ccd_synth_fused.hip): [N-1x1] [C-1x1] then up to 3 k x k layers on C channels,
// stabiliser and output transform.  All offsets index the float blob `params`.
struct SynthFused {
    const float* dense;      // [c_in][h][w]
    float* out;              // [c][h][w] synthesis output (f32) or null
    void* plane[3];          // integer planes (u8 / u16), used when write_planes
    const float* params;
    int32_t h, w, c_in, c, n_hidden;
    int32_t relu0, relu1;
    int32_t w0_off, b0_off;  // [n_hidden][CP], [n_hidden]   (CP = c_in rounded up to 4, zero padded)
    int32_t w1_off, b1_off;  // [c][n_hidden], [c]
    int32_t n_conv;
    int32_t conv_k[3], conv_residual[3], conv_relu[3], conv_w_off[3], conv_b_off[3];
    int32_t has_stab, stab_c_in, stab_w_off, stab_b_off;  // [c][CP] zero padded, [c]
    int32_t out_w_off, out_b_off;                         // [c][c], [c]
    int32_t halo;            // sum of the conv radii
    int32_t bitdepth, write_planes;
};

// Whole float path of a cool-chic in ONE kernel (ccd_fused.hip): int8 latent pyramid -> learned upsampling ->
// synthesis -> float and / or integer samples.  Nothing but the int8 grids is read from HBM.
constexpr int kFdMaxLevels = 12;     // latent levels (4K "auto" rule: 9)
constexpr int kFdMaxConv = 3;
// index of the kron product w[a] * w[b] (a, b = position folded onto the first half of the symmetric 1-D filter)
__host__ __device__ constexpr int k2_index(int a, int b) {
    return a <= b ? a * 4 - a * (a - 1) / 2 + (b - a) : b * 4 - b * (b - 1) / 2 + (a - b);
}
struct FusedDec {
    const int8_t* lat[kFdMaxLevels];  // latent (non-hyper) grids, finest first
    int32_t lh[kFdMaxLevels], lw[kFdMaxLevels];
    int32_t n_lv;
    // products of the symmetric 1-D filters, f32-rounded like the 2-D kron kernel the reference materialises
    // (upsampling.py:189-196, 312-325): k2u[i] = x2 transposed conv from level i + 1 to level i, k2p[i] = pre-concatenation
    // conv applied at level i.  10 distinct values each for k = 8 / k = 7 (k2_index).
    float k2u[kFdMaxLevels][10], k2p[kFdMaxLevels][10];
    // synthesis parameters in MFMA order (one "quad" = the 4 output-row weights of one multiply-add step), all offsets
    // in floats into `params`; the whole block [0, n_params) is staged in LDS
    const float* params;
    int32_t n_params;
    int32_t n_tiles_hidden;           // hidden units / 4 (rounded up)
    int32_t wq_off, b0_off;           // [n_tiles_hidden][NWV * 64], [n_tiles_hidden][4]
    int32_t b1_off;                   // [CT][4]
    int32_t stab_off, stabb_off;      // [NWS * 64], [CT][4]
    int32_t conv_off[kFdMaxConv], convb_off[kFdMaxConv];  // [NWC * 64], [CT][4]
    int32_t out_off, outb_off;        // [NWO * 64], [CT][4]
    int32_t h, w;                     // size of the finest latent level = size of the synthesis output
    int32_t c;                        // output channels
    int32_t relu0, relu1, n_conv, conv_residual[kFdMaxConv], conv_relu[kFdMaxConv], has_stab;
    int32_t margin;                   // halo of the tile, even, >= n_conv
    int32_t tiles_x, tiles_y;
    float* out;                       // [c][h][w] f32 or null
    void* plane[3];
    int32_t bitdepth, write_planes;
    // PRE = true instantiations: levels >= 1 evaluated once per frame by the batch's pyramid steps; channels 1 .. n_lv - 1 at the
    // resolution of level 1, f32 [n_lv - 1][lh[1]][lw[1]] (channel 1 = level 1's own latent through the 7x7 filter first)
    const float* l1;
    // common randomness (NZ = n_lv instantiations): the noise planes at full resolution, f32 [n_lv][h][w]
    const float* noise;
};

}  // namespace ccd
