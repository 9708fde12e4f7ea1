// ccd_entropy_pipe.hip - the production entropy kernel: a software pipeline inside one workgroup per
// cool-chic.  Same arithmetic as ccd_entropy.hip (the generic, barrier-phased kernel, kept as the
// fallback for networks whose operands do not fit 32 bits), restructured around what the serial
// chain costs on CDNA4: a lone wave issues one instruction every ~5 cycles and every VALU->SALU
// hand-over adds ~13 (tools/ubench/lat.hip), so
//
//   * wave 0 (the DECODER) runs nothing but the range-decoder recurrence: per symbol one LDS read of
//     a 64-entry window of cumulatives (L, P = R - L), two multiply-adds, one compare that writes EXEC
//     (the hit lane becomes the first active one: four v_readfirstlane, no lane search on the chain)
//     and ~6 scalar ops.  Symbols outside the window hit a sentinel lane whose
//     P = 0, which makes the new range 0 and so rides the (rare) renormalisation branch into the slow
//     path - no extra test on the common path;
//   * waves 1..N-1 (PRODUCERS) run ahead: for each batch of <= 16 pixels of a wavefront diagonal they
//     gather the contexts from an LDS ring of recently decoded symbols, evaluate the integer MLP with
//     4 lanes per pixel (32x32->64 multiply-adds, weights read as 16-byte LDS vectors, activations
//     exchanged through a per-wave LDS tile) and expand (mu, scale) into the window table with one
//     f64 exp per lane;
//   * hand-over through LDS words: per batch slot one ready bit per producer task ("part"), and the decoder's
//     progress as a pair (batches, pixels of the stream).  A pixel of diagonal c+1 only needs its own row's
//     pixel of diagonal c, so producers work on c+1 while the decoder is still finishing c; a batch whose
//     later parts are not built yet is decoded part by part, each part published at once;
//   * a lone wave issues in order, so every instruction between two symbols lengthens the chain: a full
//     16-symbol batch runs an unrolled copy of the symbol loop without index arithmetic, bound test or branch,
//     and the decoder stays inside ONE asm region for a whole grid (batch hand-over, step advance, renormalisation);
//   * batches are not tied to wavefront steps: the body of a wide grid (all steps of >= 23 pixels) is cut into 16-pixel batches /
//     8-pixel tasks as ONE stream of pixels (StreamBody), so every batch is full, there is no short tail batch and no step
//     hand-over; a task may hold pixels of two steps, and the decoder takes each pixel's ring cell and latent-grid offset
//     from the row meta its producer wrote (RowMeta::cell / goff) instead of keeping a geometry of its own;
//   * a batch whose parts arrive one by one is decoded part by part through unrolled 8- / 4-symbol blocks (ccd_dec_parts*.inc),
//     and every look at a ready word brings the part's top symbols and first rows along;
//   * between grids the whole workgroup computes the IFCE features of the next grid (loads requested a
//     position ahead through explicit global pointers, straight-line body: see the notes there);
//   * optionally (EntropyParams::mfma, off by default: measured slower) the ARM's layers of 8-pixel tasks run
//     on the matrix cores with operands split into signed bytes - exact, see the MF notes above producer_grid.
//
// Reference behaviour restated: bitstream/component/latent.py:18-187, armint.py:180-203,
// coolchic.py:89-169, rangecoder.py:80-94 (constriction RangeDecoder + QuantizedLaplace(-64,63)).
// The coding order (latent.py:66-140) and its walks - StepWalk, StepIter, StreamBody, grid_segments, ring_cell - are stated in
// ccd_wavefront.hpp.
#include <hip/hip_runtime.h>
#include <type_traits>

#include "ccd_device.hpp"
#include "ccd_kernels.hpp"
#include "ccd_laplace.hpp"
#include "ccd_wavefront.hpp"

namespace ccd {

// -DCCD_PIPE_PROFILE=1: light counters (per-grid totals, decoder stalls: nothing on the fast path);
// -DCCD_PIPE_PROFILE=2: + five stamps per task of producer 0 (idle / early work / late wait / late work / between tasks);
// -DCCD_PIPE_PROFILE=3: a time stamp around every phase (each costs an SMEM round trip: perturbs the pipeline).
#if defined(CCD_PIPE_PROFILE) && CCD_PIPE_PROFILE >= 3
#define PROF_T() __builtin_amdgcn_s_memtime()
#define PROF_ADD(var, t0) var += __builtin_amdgcn_s_memtime() - (t0)
#define PROF_SUB(var, t0) var -= __builtin_amdgcn_s_memtime() - (t0)
#else
#define PROF_T() 0ull
#define PROF_ADD(var, t0) (void)(t0)
#define PROF_SUB(var, t0) (void)(t0)
#endif
// level 2 only, matrix-core body: a stamp of TaskClock (the vector-ALU body's stamps are its methods)
#if defined(CCD_PIPE_PROFILE) && CCD_PIPE_PROFILE == 2 && defined(CCD_PIPE_TRACE)
#define LPROF_T(cond) __builtin_amdgcn_s_memtime()
#elif defined(CCD_PIPE_PROFILE) && CCD_PIPE_PROFILE == 2
#define LPROF_T(cond) ((cond) ? __builtin_amdgcn_s_memtime() : 0ull)
#else
#define LPROF_T(cond) 0ull
#endif
// -DCCD_PIPE_PROFILE=2 -DCCD_PIPE_TRACE: EVERY producer stamps its tasks, and the tasks of the grid whose width is g_trace_cfg[0],
// 64 steps from "g_trace_cfg[1] steps left" on, are written out as records of 8 words (tools/trace_tasks.py draws the
// time line of a few steps from them: which hand-over a step of a chain-bound grid waits for).  One stream per launch.
// The records are collected in LDS (32 bytes each, behind the kernel's own regions) and copied out when the kernel ends: a global
// store per task put every producer behind a vmcnt wait of ~2 k ticks.
#if defined(CCD_PIPE_TRACE)
constexpr int kTraceTasks = 512;  // (16 KB: the kernel's own regions take ~128 KB of the 160)
constexpr uint32_t kTraceLdsBytes = kTraceTasks * 32u;
__device__ unsigned int g_trace[kTraceTasks * 8];
__device__ unsigned int g_trace_cfg[2];
constexpr bool kProfTrace = true;
#else
constexpr bool kProfTrace = false;
#endif

// widest step of a grid >= CCD_T8 pixels: 8-pixel tasks; >= CCD_T4: 4-pixel tasks; else 2-pixel tasks (tunable at build time)
#ifndef CCD_T8
#define CCD_T8 25
#endif
#ifndef CCD_T4
#define CCD_T4 9
#endif
#ifndef CCD_PIPE_THREADS
#define CCD_PIPE_THREADS 512
#endif
constexpr int kPipeThreads = CCD_PIPE_THREADS;  // 8 waves: 1 decoder + 7 producers
constexpr int kPipeWaves = kPipeThreads / 64;
constexpr int kProducers = kPipeWaves - 1;  // (the decoder's SIMD neighbour left idle, six producers: nothing to gain, r04)
// pixels per decoder batch: 16 (two 8-pixel or four 4-pixel tasks), 8 with 2-pixel tasks (bpx / kBpx below).
// 32-pixel batches for 8-pixel tasks: bit-exact but measured slower (50.3 against 46.2 ms on kodak24, r01/r03)
constexpr int kRows = 128;                  // table rows in LDS = slots x pixels per batch (8 x 16 or 16 x 8)
// Producer task = a part of a batch: 8 pixels x 8 lanes on wide wavefronts, 4 pixels x 16 lanes on short ones
// (small grids are bound by the producers' latency, not their throughput).
constexpr int kSlots = 16;                  // most batch slots in flight (power of two)
constexpr int kMaxNV = 8;                   // MLP width <= 32 (in 4-wide vectors)
constexpr int kRingRows = 512;              // most rows of the decoded-symbol ring (>= live rows + 4; 4K: 384 + 4); a slot uses
                                            // EntropyParams::ring_rows of them (power of two >= widest grid / 10 + 6)
// Scale index up to which a 14-symbol window [round(mu) - 7, round(mu) + 6] is used (b <= 1: 99.3 % of the symbols of
// a real stream, window misses ~3e-4): four pixels' windows are then built by ONE pass of the wave.
constexpr int kNarrowMaxScale = kScaleOffset;
constexpr int kIfceFastIn = 12;             // most IFCE input channels (coarser grids) of the register-resident feature pass
constexpr unsigned kSpinLimit = 1u << 27;   // bounded spins: a lost hand-over becomes an error, not a hang

struct alignas(16) RowMeta {  // per table row (= pixel of a batch in flight)
    // (entry kRows of each array, and table row kRows, are DUMMIES: a lane with nothing to store stores there - an address select
    // instead of an exec-masked store, whose skip branch costs ~17 ticks on the producers' late path even when not taken)
    double rcp[kRows + 2];      // RN(1 / b)
    int32_t mu_idx[kRows + 2];
    int32_t top[kRows + 2];     // symbol of window lane 1
    // where the decoder's epilogue puts the pixel's symbol: LDS address of its ring cell, byte offset in the latent grid.  Written
    // by the task's producer (early part: position only), read by the decoder with the top symbols - the decoder then needs no
    // geometry of its own, and a batch may hold pixels of any steps.
    uint32_t cell[kRows + 2];
    uint32_t goff[kRows + 2];
};
static_assert(offsetof(RowMeta, cell) - offsetof(RowMeta, top) == 520 && offsetof(RowMeta, goff) - offsetof(RowMeta, top) == 1040,
              "the decoder's asm region reads cell / goff at these immediate offsets from a top symbol's address");

// The workgroup's dynamic LDS.  Regions are referred to by 32-bit byte offsets (LdsRef): a generic 64-bit pointer per
// region would pin two SGPRs each for the whole kernel (eleven regions), and the compiler could no longer see that the
// accesses are LDS accesses once a pointer travelled through a struct.
extern __shared__ __attribute__((aligned(16))) unsigned char ccd_pipe_smem[];
template <typename T>
__device__ __forceinline__ T* smem_at(uint32_t off) { return reinterpret_cast<T*>(ccd_pipe_smem + off); }
// An LDS address as a 32-bit value (one that can be pinned in a VGPR ahead of its use), and back
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) const char*)p));
}
template <typename T>
__device__ __forceinline__ __attribute__((address_space(3))) T* lds_at(uint32_t addr) {
    return reinterpret_cast<__attribute__((address_space(3))) T*>(static_cast<uintptr_t>(addr));
}
template <typename T>
struct LdsRef {
    uint32_t off;
    __device__ __forceinline__ operator T*() const { return reinterpret_cast<T*>(ccd_pipe_smem + off); }
    __device__ __forceinline__ LdsRef& operator=(T* p) {
        off = static_cast<uint32_t>(reinterpret_cast<unsigned char*>(const_cast<typename std::remove_const<T>::type*>(p)) - ccd_pipe_smem);
        return *this;
    }
};

// Byte offsets of the LDS regions (all multiples of 16).  ONE definition for the kernel's carve-up (run-time shape), the
// compile-time layout of a fixed-shape instantiation (ShapeFix) and the host's size (entropy_pipe_lds_bytes).
struct PipeLayout { uint32_t ring, w, b, act, a, tab, meta, rcp, exp, ready, consumed, abort, end; int n_w_hidden; };
__host__ __device__ constexpr PipeLayout pipe_layout(int dim, int n_layers, int in_pad, int ring_rows, int mf_tabs) {
    PipeLayout L{};
    L.ring = 0;  // LDS address 0: the decoder uses ring cells as addresses
    L.w = static_cast<uint32_t>(ring_rows) * 64u;  // network next: its addresses stay below 64 KB, so the per-vector offsets fold into the ds_read immediates
    L.n_w_hidden = (n_layers - 1) * dim * in_pad;
    const int n_w_total = L.n_w_hidden + 4 * in_pad;  // + output layer (2 rows) + stabiliser (2 rows)
    L.b = L.w + static_cast<uint32_t>((n_w_total + 3) & ~3) * 4u;
    const int n_b_total = (n_layers - 1) * dim + 4;
    L.act = L.b + static_cast<uint32_t>((n_b_total + 1) & ~1) * 8u;
    L.a = L.act + static_cast<uint32_t>(kProducers * ((mf_tabs ? 16 : 8) * in_pad + 4)) * 4u;
    L.tab = L.a + static_cast<uint32_t>(mf_tabs) * 1024u;
    L.meta = L.tab + static_cast<uint32_t>(kRows + 1) * 64u * 8u;
    L.rcp = L.meta + static_cast<uint32_t>(sizeof(RowMeta));
    L.exp = L.rcp + static_cast<uint32_t>(kNumScale + 1) * 8u;
    L.ready = L.exp + static_cast<uint32_t>(1 << CCD_EXP_LOG) * 8u;
    L.consumed = L.ready + static_cast<uint32_t>(kSlots) * 4u;
    L.abort = L.consumed + 8u;
    L.end = (L.ready + static_cast<uint32_t>(kSlots + 8) * 4u + 15u) & ~15u;
    return L;
}

// Shape of the ARM as the producers see it.  ShapeDyn: read from the parameter block (any network the kernel supports).
// ShapeFix: compile-time inputs / layers / spatial contexts - every LDS region of the task loop sits at a constant address (no
// scalar registers held for offsets, so no SGPR spill moves on the late path), the hidden-layer loop has a constant trip
// count and the `n_layers` / `split` branches are gone.  Instantiated for the architecture the metric's sets use
// (cfg/dec/intra/hop.cfg: 14 spatial contexts + 6 IFCE features, two hidden layers); the left neighbour (y, x - 1) is the
// context of priority 0 (arm.py:501-509), i.e. input 0 of every network with a spatial context.
struct ShapeDyn { static constexpr bool fixed = false; static constexpr int dim = 0, n_layers = 0, n_sp = 0; };
template <int DIM, int NL, int NSP>
struct ShapeFix { static constexpr bool fixed = true; static constexpr int dim = DIM, n_layers = NL, n_sp = NSP; };
using ShapeHop = ShapeFix<20, 3, 14>;
// (r06: ShapeFix<8, 3, 6> = intra/lop.cfg, the I frames of the 1080p GOP, was built and measured: 164.85 against 163.98 ms for the
// GOP's cool-chics, kodak24_hq 39.58 against 39.4 - nothing; a two-vector network has no register pressure to relieve.  Not kept.)

// The IFCE features of one position of the previous grid sit NEXT to each other in the int16 scratch (position-major, stride =
// the number of features: 12 bytes for the usual six): a task's feature reads touch one cache line per pixel instead of one per
// pixel and feature, and ten neighbouring positions (ten wavefront steps) share that line.  r03 kept one plane per feature:
// 6 x 52 lines per step of a Kodak grid 0 = 40 KB through a 16 KB L1, every read an L2 round trip.  Same bytes written either
// way (a power-of-two stride was tried: + 27 % HBM traffic for nothing).  The int32 side plane of the dynamic operand check stays
// planar: it is never read on real streams.
__host__ __device__ constexpr int feat_stride(int n_if) { return n_if > 0 ? n_if : 1; }

struct PipeCtx {
    const EntropyParams* P;
    LdsRef<uint2> s_tab;          // [kRows][64] (L, P)
    LdsRef<RowMeta> s_meta;
    LdsRef<const double> s_rcp;   // [kNumScale] RN(1 / b), b = the float32 Laplace scale of the index, widened: LDS copy of the table
                                  // (a global load per pixel would put an L2 round trip on every task's critical path)
    LdsRef<const double> s_exp;   // [128] 2^(j/128), the table of exp_nonpos
    LdsRef<int32_t> s_w;          // transposed int32 weights Wt[out][in_pad]
    LdsRef<int64_t> s_b;          // biases: hidden layers, output (2), stabiliser (2)
    LdsRef<int32_t> s_act;        // [kProducers][8][in_pad] (a task holds at most 8 pixels); [kProducers][16][in_pad] with MF
    LdsRef<uint32_t> s_a;         // MF: A operands [mf_tables][64] x 16 bytes
    LdsRef<int8_t> s_ring;        // [ring_mask + 1][64]
    LdsRef<uint32_t> s_ready;     // [kSlots] one bit per part (producer task) of the slot's batch whose table rows are complete
                                  // (set by the producers, cleared by the decoder)
    LdsRef<uint32_t> s_consumed;  // [0] batches, [1] pixels of the stream whose symbols the decoder has published (ring + counters)
    LdsRef<uint32_t> s_abort;
    int dim, n_layers, n_sp, n_if, n_w_hidden;
    int ring_mask;         // ring rows - 1
#if defined(CCD_PIPE_TRACE)
    uint32_t trace_off;    // LDS offset of the trace records
#endif
    // per grid
    int H, W, fin, fh, fw;
    int fstride;           // feat_stride(n_if)
    int task_pix;          // pixels per producer task in this grid (8, 4 or 2)
    int k_left;            // index of the context (y, x - 1) among the spatial contexts, -1 if the mask has none
    int8_t* lat;
    uint32_t seq_base;     // batches / pixels of the grids decoded so far
    uint32_t px_base;
};

struct DecState {
    uint64_t dist, range;  // dist = point - lower (all the decoder ever uses)
    uint32_t word_pos, wbase, wbuf;
    uint64_t n_decoded;
    uint32_t n_part_batches;  // batches decoded part by part (status word 37)
    unsigned long long prof_wait, prof_work, stall_ticks, stall_events, n_rare, n_search, n_spins;
    unsigned long long wait_by_j[6];  // grid 0, steps with n >= 64: decoder wait per batch position
};

__device__ __forceinline__ void lds_write_release(uint32_t* p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// All lanes read the same word; readfirstlane tells the compiler the result is wave-uniform so that the
// control flow hanging off it (and every value defined inside) stays scalar.
__device__ __forceinline__ uint32_t lds_load_acquire(const uint32_t* p) {
    return __builtin_amdgcn_readfirstlane(__hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
}

// Pointers read from the parameter block are generic: their loads / stores compile to FLAT instructions, which count on
// lgkmcnt as well as vmcnt - so every later LDS wait (the hand-over flags!) also waited for the global access to
// complete.  An explicit global address space gives global_load / global_store (vmcnt only).
template <typename T> using glb_ptr = T __attribute__((address_space(1)))*;

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uni(uint64_t v) {
    return (static_cast<uint64_t>(uni(static_cast<uint32_t>(v >> 32))) << 32) | uni(static_cast<uint32_t>(v));
}

// Spin until *p >= want (sequence numbers only grow). Returns false on abort / timeout.
// (the wanted values are wave-uniform but reach these functions in vector registers: stated scalar here, or every poll compares
// on the vector ALU and branches on VCC.  The first look is kept apart from the loop: where the producers are the limit it
// succeeds, and the loop's exit bookkeeping stays off that path.)
__device__ __forceinline__ bool wait_ge(const uint32_t* p, uint32_t want_v, uint32_t* s_abort) {
    const uint32_t want = uni(want_v);
    if (__builtin_expect(static_cast<int32_t>(lds_load_acquire(p) - want) >= 0, 1)) return true;
    unsigned spins = 0;
    while (static_cast<int32_t>(lds_load_acquire(p) - want) < 0) {
        // no s_sleep: the waits of this pipeline are short, and waking up costs more than the polling LDS reads (measured)
        if ((++spins & 1023u) == 0) {
            if (lds_load_acquire(s_abort) != 0) return false;
            if (spins > kSpinLimit) { lds_write_release(s_abort, static_cast<uint32_t>(-CCD_ERR_HIP)); return false; }
        }
    }
    return true;
}

// The decoder's progress is a pair (batches, pixels) in one aligned 64-bit LDS word: one read serves both conditions.
__device__ __forceinline__ bool progress_reached(const uint32_t* p, uint32_t want_batches, uint32_t want_pixels) {
    const uint64_t v = uni(__hip_atomic_load(reinterpret_cast<const uint64_t*>(p), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
    // (| of two sign bits, not &&: one scalar test)
    return static_cast<int32_t>((static_cast<uint32_t>(v) - want_batches) | (static_cast<uint32_t>(v >> 32) - want_pixels)) >= 0;
}
__device__ __forceinline__ bool wait_ge2(const uint32_t* p, uint32_t want_batches_v, uint32_t want_pixels_v, uint32_t* s_abort) {
    const uint32_t want_batches = uni(want_batches_v), want_pixels = uni(want_pixels_v);
    if (__builtin_expect(progress_reached(p, want_batches, want_pixels), 1)) return true;
    unsigned spins = 0;
    while (!progress_reached(p, want_batches, want_pixels)) {
        if ((++spins & 1023u) == 0) {
            if (lds_load_acquire(s_abort) != 0) return false;
            if (spins > kSpinLimit) { lds_write_release(s_abort, static_cast<uint32_t>(-CCD_ERR_HIP)); return false; }
        }
    }
    return true;
}

// =================================================================================================
// DECODER (wave 0): one grid.  Returns the batch sequence number after the grid.
// =================================================================================================
template <bool MF>
__device__ __forceinline__ uint32_t decoder_grid(const PipeCtx& C, DecState& S) {
    const int lane = threadIdx.x & 63;
    const EntropyParams& P = *C.P;
    // Everything that steers the decoder is wave-uniform; `uni` (readfirstlane) states it to the compiler,
    // which otherwise treats values loaded through the parameter block as divergent and moves the whole
    // recurrence to VGPRs with exec-mask control flow.
    StepIter it;
    it.init(uni(C.H), uni(C.W));
    uint32_t seq = uni(C.seq_base);
    uint64_t rc_dist = uni(S.dist), rc_range = uni(S.range);
    uint32_t word_pos = uni(S.word_pos), wbase = uni(S.wbase), wbuf = S.wbuf;
    const uint32_t n_words = uni(P.n_words);
    const glb_ptr<const uint32_t> words_g = (glb_ptr<const uint32_t>)P.words;
    int task_pix = uni(C.task_pix);  // (of the grid; the ramps around a streamed body run smaller tasks: per segment below)
    const int grid_w = uni(C.W);
    // pixels per batch: 16 (two 8-pixel or four 4-pixel tasks) or 8 (four 2-pixel tasks).  32-pixel batches were tried twice
    // (r01; r03 with the first half published half-way): fewer hand-overs for the decoder, but slower overall.
    const uint32_t bpx_shift = task_pix == 2 ? 3u : 4u;
    const int bpx = task_pix == 2 ? 8 : 16;
    const int slot_mask = kRows / bpx - 1;       // 8 / 16 slots share the 128 table rows
    int task_shift = task_pix == 8 ? 3 : (task_pix == 4 ? 2 : 1);
    // LDS byte addresses (the dynamic LDS starts at 0) and per-lane constants of the step loop below
    const uint32_t ready_base = C.s_ready.off;  // s_consumed sits kSlots words behind it, the ring at LDS address 0 (kernel set-up)
    const uint32_t top_base = C.s_meta.off + static_cast<uint32_t>(offsetof(RowMeta, top));
    const uint32_t tab_lane = C.s_tab.off + static_cast<uint32_t>(lane) * 8u;
    const uint32_t lane_top_off = top_base + static_cast<uint32_t>(lane & (bpx - 1)) * 4u;
    const uint64_t lat_addr = uni(reinterpret_cast<uint64_t>(C.lat));
    const RowMeta& meta = *C.s_meta;
    bool ok = true;
    int raw = 0, top_l = 0;  // lane p: window lane chosen for / top symbol of pixel p of the current batch
    uint32_t n_spins = 0;    // polls of a ready counter inside the asm region (profile builds report them)
    uint32_t pix0 = uni(C.px_base);  // pixels of the stream decoded before the current step (the asm region counts on)
    uint32_t n_part = 0;             // batches decoded part by part
    // segments of the grid (grid_segments): a step of a raster-order grid comes back after every step
    GridSeg segs[3];
    const int n_segs = grid_segments(static_cast<uint32_t>(it.H), static_cast<uint32_t>(it.W), uni(C.task_pix), segs);
    int seg_i = 0, seg_c = 0;
    while (ok && seg_c < it.n_steps) {
        while (seg_i + 1 < n_segs && seg_c >= static_cast<int>(segs[seg_i].first + segs[seg_i].steps)) ++seg_i;
        const bool seg_body = segs[seg_i].body;
        const int seg_steps = it.raster ? 1 : static_cast<int>(segs[seg_i].steps);
        const uint32_t seg_n_pix = uni(segs[seg_i].n_pix);
        task_pix = uni(segs[seg_i].task_pix);
        task_shift = task_pix == 8 ? 3 : (task_pix == 4 ? 2 : 1);
        it.seek(seg_c);
        seg_c += seg_steps;
        // ---- one wavefront step = one asm region: per batch the ready check, the symbol loop (hand-scheduled recurrence, see
        // the file header) and the epilogue (symbols -> LDS ring + latent grid, slot handed back, progress published) without
        // returning to compiled code.  It leaves early for a symbol whose new range has a zero high word (renormalisation,
        // window miss, invalid data: status 1, handled below, then re-entered) and for a batch that is not ready (status 2).
        // The region walks the remaining steps of a wavefront-ordered grid itself (label 30); `it` only sets it up.  A grid
        // narrower than 10 (raster order, one pixel per step) comes back after every step.
        uint32_t n_step = seg_body ? seg_n_pix : static_cast<uint32_t>(it.n), step_x0 = static_cast<uint32_t>(it.x0), step_hy = static_cast<uint32_t>(it.H - it.y0);
        uint32_t steps_left = (it.raster || seg_body) ? 1u : static_cast<uint32_t>(seg_steps);
        uint32_t i = 0, mode = 0;
        // lane p <-> pixel p of the current batch: LDS address of its ring cell, its byte in the latent grid (RowMeta::cell / goff,
        // read with the batch's top symbols)
        uint32_t v_ring = 0, v_goff = 0;
        while (true) {
            uint32_t status, k_rare;
            i = uni(i); seq = uni(seq); mode = uni(mode); n_spins = uni(n_spins);  // scalar operands of the region below
            n_step = uni(n_step); step_x0 = uni(step_x0); step_hy = uni(step_hy); steps_left = uni(steps_left); pix0 = uni(pix0);
            n_part = uni(n_part);
// (this region names m0 in its clobber list on purpose - it uses m0 and restores nothing; the diagnostic is silenced for this
// statement only: every other asm statement of the file keeps its inline-asm warnings)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
            asm volatile(
                "s_mov_b64 s[50:51], %[dst]\n\t"
                "s_mov_b64 s[52:53], %[rng]\n\t"
                "s_lshl_b32 s69, 1, %[bshift]\n\t"   // pixels per batch
                "s_sub_u32 s62, s69, 1\n\t"
                "s_lshl_b32 s70, 1, %[tshift]\n\t"
                "s_sub_u32 s70, s70, 1\n\t"           // pixels per task - 1
                "s_sub_u32 s64, %[gw], 10\n\t"        // W - kWfSlope: x0 of a step that starts a row (StepWalk::next)
                "s_mov_b32 s65, 0\n\t"               // 1: the batch is decoded part by part (see 27:)
                "s_cmp_eq_u32 s69, 16\n\t"
                "s_cselect_b32 s61, 1, 0\n\t"
                "s_mul_i32 s72, %[n], s61\n\t"       // steps shorter than i + 16 have no full batch ahead; 0: no unrolled block on this grid
                "s_lshr_b32 s73, 16, %[tshift]\n\t"
                "s_bfm_b32 s73, s73, 0\n\t"          // ready word of a full 16-symbol batch
                "s_cmp_eq_u32 %[mode], 0\n\t"
                "s_cbranch_scc0 6f\n\t"
                // ---- batch start: symbol index i is the first of a batch
                "5:\n\t"
                "s_add_u32 s54, %[i], s69\n\t"
                "s_min_u32 s54, s54, %[n]\n\t"
                "s_and_b32 s55, %[seq], %[smask]\n\t"
                "v_lshl_add_u32 v51, s55, 2, %[rdy]\n\t"
                "s_lshl_b32 s56, s55, %[bshift]\n\t"
                "s_sub_u32 s57, s54, %[i]\n\t"
                "s_add_u32 s57, s57, s70\n\t"
                "s_lshr_b32 s57, s57, %[tshift]\n\t"
                "s_bfm_b32 s57, s57, 0\n\t"          // one bit per part (producer task) of the batch
                "v_lshl_add_u32 v50, s56, 9, %[tabl]\n\t"
                "v_lshl_add_u32 v53, s56, 2, %[l4]\n\t"
                "s_mov_b32 s68, 0\n\t"
                "s_branch 18f\n\t"
                // bounded spin on the slot's counter (short waits are the rule on short steps); a long wait goes back to the
                // compiled code, which also watches the abort flag.  Every look asks for the counter AND, behind it, for what the
                // first symbols need (top symbols, first two rows): LDS answers a wave in order and a producer stores its rows
                // before it counts its part in, so a counter that reads "there" vouches for the answers behind it - the look that
                // succeeds costs ONE LDS round trip, not two (r04: ~150 ticks per part where the producers are the limit)
                "11:\n\t"
                "s_add_u32 s68, s68, 1\n\t"
                "s_cmp_lt_u32 s68, 1024\n\t"
                "s_cbranch_scc0 7f\n\t"
                "18:\n\t"
                "ds_read_b32 v52, v51\n\t"
                "ds_read_b32 %[top], v53\n\t"
                "ds_read_b32 %[ring], v53 offset:520\n\t"
                "ds_read_b32 %[goff], v53 offset:1040\n\t"
                "ds_read2st64_b64 v[40:43], v50 offset1:1\n\t"
                "s_waitcnt lgkmcnt(4)\n\t"
                "v_readfirstlane_b32 s58, v52\n\t"
                "s_cmp_eq_u32 s58, s57\n\t"
                "s_cbranch_scc1 13f\n\t"
                "s_bitcmp1_b32 s58, 0\n\t"
                "s_cbranch_scc0 11b\n\t"
                // the first part is there, the rest is not: the producers are the limit here.  Decode the batch part by part - each
                // part as soon as its producer is done - and publish every part's symbols at once, so that the producers of the
                // NEXT step start on a part while the later parts of this step are still being decoded (a step then costs
                // "table latency + one part" instead of "table latency + the whole step")
                "s_add_u32 %[spins], %[spins], s68\n\t"
                "s_add_u32 %[npart], %[npart], 1\n\t"
                "s_mov_b32 s65, 1\n\t"
                "s_mov_b32 s66, s54\n\t"
                "s_mov_b32 s67, %[i]\n\t"           // (what 27: sets for a part that starts at symbol i; its rows are the batch's first)
                "s_add_u32 s54, %[i], s70\n\t"
                "s_add_u32 s54, s54, 1\n\t"
                "s_min_u32 s54, s54, s66\n\t"
                "s_sub_u32 s58, s54, %[i]\n\t"     // a full 8-symbol part (8-pixel tasks): its unrolled block (ccd_dec_parts8.inc)
                "s_cmp_eq_u32 s58, 8\n\t"
                "s_cbranch_scc1 400f\n\t"
                "s_cmp_eq_u32 s58, 4\n\t"          // a 4-symbol part (4-pixel tasks): ccd_dec_parts4.inc
                "s_cbranch_scc1 440f\n\t"
                "s_branch 31f\n\t"
                "8:\n\t"
                "ds_read2st64_b64 v[40:43], v50 offset1:1\n\t"
                "s_branch 19f\n\t"
                "13:\n\t"
                "s_add_u32 %[spins], %[spins], s68\n\t"
                // a full batch of 16 symbols takes the unrolled copy of the loop (80:): no loop control on the chain
                "19:\n\t"
                "s_sub_u32 s58, s54, %[i]\n\t"
                "s_cmp_eq_u32 s58, 16\n\t"
                "s_cbranch_scc1 80f\n\t"
                // a look leaves rows 0 / 1 in flight as ONE read (both in v[40:43]); the loop's copies count single reads, so whoever
                // enters the loop behind a look waits for that read here (the unrolled blocks count it themselves)
                "31:\n\t"
                "s_waitcnt lgkmcnt(0)\n\t"
                ".p2align 6\n\t"
                "1:\n\t"
                // ---- copy 0: (L, P) of the current symbol in v[40:41], two rows ahead in flight (order: dloop_variants.hip)
                "s_lshr_b64 s[40:41], s[52:53], 24\n\t"
                "ds_read_b64 v[46:47], v50 offset:1024\n\t"
                "s_waitcnt lgkmcnt(2)\n\t"
                "v_mad_u64_u32 v[44:45], s[42:43], s40, v40, 0\n\t"
                "v_mad_u32_u24 v45, v40, s41, v45\n\t"
                "v_cmpx_ge_u64 vcc, s[50:51], v[44:45]\n\t"
                "v_mad_u64_u32 v[48:49], s[42:43], s40, v41, 0\n\t"
                "v_mad_u32_u24 v49, v41, s41, v49\n\t"
                "s_and_b32 m0, %[i], s62\n\t"
                "s_ff1_i32_b64 s44, vcc\n\t"
                "v_readfirstlane_b32 s48, v48\n\t"
                "v_readfirstlane_b32 s49, v49\n\t"
                "v_readfirstlane_b32 s46, v44\n\t"
                "v_readfirstlane_b32 s47, v45\n\t"
                "s_mov_b64 exec, -1\n\t"
                "s_cmp_eq_u32 s49, 0\n\t"
                "s_cbranch_scc1 40f\n\t"
                "s_mov_b64 s[52:53], s[48:49]\n\t"
                "s_sub_u32 s50, s50, s46\n\t"
                "s_subb_u32 s51, s51, s47\n\t"
                "v_writelane_b32 %[raw], s44, m0\n\t"
                "s_add_u32 %[i], %[i], 1\n\t"
                "s_cmp_lt_u32 %[i], s54\n\t"
                "s_cbranch_scc0 2f\n\t"
                "16:\n\t"
                // ---- copy 1: (L, P) of the current symbol in v[42:43], two rows ahead in flight (order: dloop_variants.hip)
                "s_lshr_b64 s[40:41], s[52:53], 24\n\t"
                "ds_read_b64 v[40:41], v50 offset:1536\n\t"
                "s_waitcnt lgkmcnt(2)\n\t"
                "v_mad_u64_u32 v[44:45], s[42:43], s40, v42, 0\n\t"
                "v_mad_u32_u24 v45, v42, s41, v45\n\t"
                "v_cmpx_ge_u64 vcc, s[50:51], v[44:45]\n\t"
                "v_mad_u64_u32 v[48:49], s[42:43], s40, v43, 0\n\t"
                "v_mad_u32_u24 v49, v43, s41, v49\n\t"
                "s_and_b32 m0, %[i], s62\n\t"
                "s_ff1_i32_b64 s44, vcc\n\t"
                "v_readfirstlane_b32 s48, v48\n\t"
                "v_readfirstlane_b32 s49, v49\n\t"
                "v_readfirstlane_b32 s46, v44\n\t"
                "v_readfirstlane_b32 s47, v45\n\t"
                "s_mov_b64 exec, -1\n\t"
                "s_cmp_eq_u32 s49, 0\n\t"
                "s_cbranch_scc1 41f\n\t"
                "s_mov_b64 s[52:53], s[48:49]\n\t"
                "s_sub_u32 s50, s50, s46\n\t"
                "s_subb_u32 s51, s51, s47\n\t"
                "v_writelane_b32 %[raw], s44, m0\n\t"
                "s_add_u32 %[i], %[i], 1\n\t"
                "s_cmp_lt_u32 %[i], s54\n\t"
                "s_cbranch_scc0 2f\n\t"
                "17:\n\t"
                // ---- copy 2: (L, P) of the current symbol in v[46:47], two rows ahead in flight (order: dloop_variants.hip)
                "s_lshr_b64 s[40:41], s[52:53], 24\n\t"
                "ds_read_b64 v[42:43], v50 offset:2048\n\t"
                "s_waitcnt lgkmcnt(2)\n\t"
                "v_mad_u64_u32 v[44:45], s[42:43], s40, v46, 0\n\t"
                "v_mad_u32_u24 v45, v46, s41, v45\n\t"
                "v_cmpx_ge_u64 vcc, s[50:51], v[44:45]\n\t"
                "v_mad_u64_u32 v[48:49], s[42:43], s40, v47, 0\n\t"
                "v_mad_u32_u24 v49, v47, s41, v49\n\t"
                "s_and_b32 m0, %[i], s62\n\t"
                "s_ff1_i32_b64 s44, vcc\n\t"
                "v_readfirstlane_b32 s48, v48\n\t"
                "v_readfirstlane_b32 s49, v49\n\t"
                "v_readfirstlane_b32 s46, v44\n\t"
                "v_readfirstlane_b32 s47, v45\n\t"
                "s_mov_b64 exec, -1\n\t"
                "s_cmp_eq_u32 s49, 0\n\t"
                "s_cbranch_scc1 42f\n\t"
                "s_mov_b64 s[52:53], s[48:49]\n\t"
                "s_sub_u32 s50, s50, s46\n\t"
                "s_subb_u32 s51, s51, s47\n\t"
                "v_writelane_b32 %[raw], s44, m0\n\t"
                "s_add_u32 %[i], %[i], 1\n\t"
                "v_add_u32 v50, 0x600, v50\n\t"
                "s_cmp_lt_u32 %[i], s54\n\t"
                "s_cbranch_scc1 1b\n\t"
                // ---- batch end of the loop above (a partial batch, or one that left the unrolled block).  FIRST what the producers
                // wait for: the symbols into the LDS ring (and the latent grid), the slot's counter back to zero (before anybody may
                // count a part of its next batch in), progress published - a producer task's late part hangs on `consumed`, and
                // where the producers are the limit (every short-step grid, grid 0 of a portrait picture) each tick between the
                // last symbol and this store is a tick of the critical path.  The ring sits at LDS address 0 (ring cell = address),
                // v51 still holds the batch's counter address, `consumed` lives kSlots words behind the counters.
                "2:\n\t"
                "s_cmp_eq_u32 s65, 0\n\t"
                "s_cbranch_scc0 26f\n\t"
                "s_sub_u32 s58, s54, 1\n\t"
                "s_and_b32 s58, s58, s62\n\t"
                "s_add_u32 s58, s58, 1\n\t"
                "s_bfm_b64 exec, s58, 0\n\t"          // lanes below the batch's pixel count
                "v_sub_u32 v52, %[top], %[raw]\n\t"
                "v_add_u32 v52, 1, v52\n\t"
                "ds_write_b8 %[ring], v52\n\t"
                "global_store_byte %[goff], v52, %[lat]\n\t"
                "s_mov_b64 exec, -1\n\t"
                "ds_write_b32 v51, %[zero]\n\t"
                "s_add_u32 %[seq], %[seq], 1\n\t"
                "s_add_u32 s58, %[pix0], %[i]\n\t"
                "v_mov_b32 v56, %[seq]\n\t"
                "v_mov_b32 v57, s58\n\t"
                "ds_write_b64 %[rdy], v[56:57] offset:64\n\t"   // batches done, pixels done (of the whole stream)
                "s_branch 22f\n\t"
                // ---- part by part: symbols [s67, i) of the step are decoded and not published yet
                "26:\n\t"
                "s_and_b32 s58, s67, s62\n\t"
                "s_sub_u32 s59, %[i], s67\n\t"
                "s_bfm_b64 exec, s59, s58\n\t"
                "v_sub_u32 v52, %[top], %[raw]\n\t"
                "v_add_u32 v52, 1, v52\n\t"
                "ds_write_b8 %[ring], v52\n\t"
                "global_store_byte %[goff], v52, %[lat]\n\t"
                "s_mov_b64 exec, -1\n\t"
                "s_add_u32 s58, %[pix0], %[i]\n\t"
                "v_mov_b32 v52, s58\n\t"
                "ds_write_b32 %[rdy], v52 offset:68\n\t"
                "126:\n\t"
                "s_cmp_lt_u32 %[i], s66\n\t"
                "s_cbranch_scc0 29f\n\t"
                // the next part of the batch starts at symbol i: it runs through the loop above like a short batch.  Wait for its bit -
                // each look with the part's top symbols and first two rows behind it, as at 11:
                "s_and_b32 s59, %[i], s62\n\t"
                "s_add_u32 s58, s59, s56\n\t"
                "v_lshl_add_u32 v50, s58, 9, %[tabl]\n\t"
                "s_lshr_b32 s59, s59, %[tshift]\n\t"
                "s_mov_b32 s67, %[i]\n\t"
                "s_add_u32 s54, %[i], s70\n\t"
                "s_add_u32 s54, s54, 1\n\t"
                "s_min_u32 s54, s54, s66\n\t"
                "s_mov_b32 s68, 0\n\t"
                "28:\n\t"
                "ds_read_b32 v52, v51\n\t"
                "ds_read_b32 %[top], v53\n\t"
                "ds_read_b32 %[ring], v53 offset:520\n\t"
                "ds_read_b32 %[goff], v53 offset:1040\n\t"
                "ds_read2st64_b64 v[40:43], v50 offset1:1\n\t"
                "s_waitcnt lgkmcnt(4)\n\t"
                "v_readfirstlane_b32 s58, v52\n\t"
                "s_bitcmp1_b32 s58, s59\n\t"
                "s_cbranch_scc1 27f\n\t"
                "s_add_u32 s68, s68, 1\n\t"
                "s_cmp_lt_u32 s68, 1024\n\t"
                "s_cbranch_scc1 28b\n\t"
                "s_branch 7f\n\t"
                "27:\n\t"
                "s_add_u32 %[spins], %[spins], s68\n\t"
                "s_sub_u32 s58, s54, %[i]\n\t"     // the second 8-symbol part of a 16-pixel batch: its unrolled block
                "s_cmp_eq_u32 s58, 8\n\t"
                "s_cbranch_scc1 420f\n\t"
                "s_cmp_eq_u32 s58, 4\n\t"          // a 4-symbol part at pixel 4, 8 or 12 of the batch
                "s_cbranch_scc0 31b\n\t"
                "s_and_b32 s58, %[i], s62\n\t"
                "s_cmp_eq_u32 s58, 4\n\t"
                "s_cbranch_scc1 450f\n\t"
                "s_cmp_eq_u32 s58, 8\n\t"
                "s_cbranch_scc1 460f\n\t"
                "s_cmp_eq_u32 s58, 12\n\t"
                "s_cbranch_scc1 470f\n\t"
                "s_branch 31b\n\t"
                // the batch is finished (its last part is published): slot handed back, batch counted
                "29:\n\t"
                "s_mov_b32 s65, 0\n\t"
                "ds_write_b32 v51, %[zero]\n\t"
                "s_add_u32 %[seq], %[seq], 1\n\t"
                "v_mov_b32 v52, %[seq]\n\t"
                "ds_write_b32 %[rdy], v52 offset:64\n\t"
                "s_branch 22f\n\t"
                // ---- re-entry after a symbol decoded by the C++ path: i already points behind it
                "6:\n\t"
                "s_sub_u32 s58, %[i], 1\n\t"
                "s_sub_u32 s57, s69, 1\n\t"
                "s_andn2_b32 s58, s58, s57\n\t"
                "s_add_u32 s54, s58, s69\n\t"
                "s_min_u32 s54, s54, %[n]\n\t"
                "s_and_b32 s55, %[seq], %[smask]\n\t"
                "v_lshl_add_u32 v51, s55, 2, %[rdy]\n\t"
                "s_lshl_b32 s56, s55, %[bshift]\n\t"
                "s_sub_u32 s57, %[i], s58\n\t"
                "s_add_u32 s57, s57, s56\n\t"
                "s_lshl_b32 s57, s57, 9\n\t"
                "v_add_u32 v50, s57, %[tabl]\n\t"
                "v_lshl_add_u32 v53, s56, 2, %[l4]\n\t"
                // whatever the batch was doing before, it goes on part by part: everything decoded so far is (re)published at
                // the end of the part that holds symbol i - 1
                "s_mov_b32 s65, 1\n\t"
                "s_mov_b32 s66, s54\n\t"
                "s_mov_b32 s67, s58\n\t"
                "s_sub_u32 s57, %[i], 1\n\t"
                "s_or_b32 s57, s57, s70\n\t"
                "s_add_u32 s57, s57, 1\n\t"
                "s_min_u32 s54, s57, s66\n\t"
                "s_mov_b32 s68, 0\n\t"
                "s_cmp_lt_u32 %[i], s54\n\t"
                "s_cbranch_scc1 8b\n\t"
                "s_branch 2b\n\t"
                "7:\n\t"
                "s_mov_b32 %[st], 2\n\t"
                "s_branch 4f\n\t"
                // ---- new range below 2^32 (one block per copy of the loop).  A zero range is a sentinel lane (window miss /
                // invalid data): compiled path.  Otherwise it is an ordinary renormalisation (constriction: state <<= 32, next
                // word shifted in), done here: commit the symbol, take the word from the 64-word buffer (a lane of `wbuf`) and go
                // on with the next copy of the loop - its rows are already in flight.
                "40:\n\t"
                "s_cmp_eq_u32 s48, 0\n\t"
                "s_cbranch_scc1 14f\n\t"
                "s_sub_u32 s50, s50, s46\n\t"
                "s_subb_u32 s51, s51, s47\n\t"
                "s_and_b32 m0, %[i], s62\n\t"
                "v_writelane_b32 %[raw], s44, m0\n\t"
                "s_add_u32 %[i], %[i], 1\n\t"
                "s_sub_u32 s58, %[wpos], %[wbase]\n\t"
                "s_and_b32 s58, s58, 63\n\t"
                "v_readlane_b32 s57, %[wbuf], s58\n\t"
                "s_mov_b32 s51, s50\n\t"
                "s_mov_b32 s50, s57\n\t"
                "s_mov_b32 s53, s48\n\t"
                "s_mov_b32 s52, 0\n\t"
                "s_add_u32 %[wpos], %[wpos], 1\n\t"
                "s_cmp_eq_u32 s58, 63\n\t"
                "s_cbranch_scc1 15f\n\t"
                "s_cmp_lt_u32 %[i], s54\n\t"
                "s_cbranch_scc0 2b\n\t"
                "s_branch 16b\n\t"
                "41:\n\t"
                "s_cmp_eq_u32 s48, 0\n\t"
                "s_cbranch_scc1 14f\n\t"
                "s_sub_u32 s50, s50, s46\n\t"
                "s_subb_u32 s51, s51, s47\n\t"
                "s_and_b32 m0, %[i], s62\n\t"
                "v_writelane_b32 %[raw], s44, m0\n\t"
                "s_add_u32 %[i], %[i], 1\n\t"
                "s_sub_u32 s58, %[wpos], %[wbase]\n\t"
                "s_and_b32 s58, s58, 63\n\t"
                "v_readlane_b32 s57, %[wbuf], s58\n\t"
                "s_mov_b32 s51, s50\n\t"
                "s_mov_b32 s50, s57\n\t"
                "s_mov_b32 s53, s48\n\t"
                "s_mov_b32 s52, 0\n\t"
                "s_add_u32 %[wpos], %[wpos], 1\n\t"
                "s_cmp_eq_u32 s58, 63\n\t"
                "s_cbranch_scc1 15f\n\t"
                "s_cmp_lt_u32 %[i], s54\n\t"
                "s_cbranch_scc0 2b\n\t"
                "s_branch 17b\n\t"
                "42:\n\t"
                "s_cmp_eq_u32 s48, 0\n\t"
                "s_cbranch_scc1 14f\n\t"
                "s_sub_u32 s50, s50, s46\n\t"
                "s_subb_u32 s51, s51, s47\n\t"
                "s_and_b32 m0, %[i], s62\n\t"
                "v_writelane_b32 %[raw], s44, m0\n\t"
                "s_add_u32 %[i], %[i], 1\n\t"
                "s_sub_u32 s58, %[wpos], %[wbase]\n\t"
                "s_and_b32 s58, s58, 63\n\t"
                "v_readlane_b32 s57, %[wbuf], s58\n\t"
                "s_mov_b32 s51, s50\n\t"
                "s_mov_b32 s50, s57\n\t"
                "s_mov_b32 s53, s48\n\t"
                "s_mov_b32 s52, 0\n\t"
                "s_add_u32 %[wpos], %[wpos], 1\n\t"
                "s_cmp_eq_u32 s58, 63\n\t"
                "s_cbranch_scc1 15f\n\t"
                "v_add_u32 v50, 0x600, v50\n\t"
                "s_cmp_lt_u32 %[i], s54\n\t"
                "s_cbranch_scc0 2b\n\t"
                "s_branch 1b\n\t"
                // ---- a full 16-symbol batch, unrolled: the three copies of the loop above in rotation without the index arithmetic, the
                // bound test and the branch (a lone wave issues in order: every instruction between two symbols lengthens the chain);
                // rows are addressed with immediate offsets from the batch's first row.  Anything unusual (renormalisation, sentinel)
                // leaves through a trampoline that restores the loop's conventions (i, v50, range registers) and continues in the loop.
                // r03 (tools/ubench/dloop_spec_alt.hip: 132.3 against 143.8 ticks per symbol): the lane search writes EXEC
                // (v_cmpx; the e32 form also writes VCC) and four v_readfirstlane take the hit lane's products - no s_ff1 ->
                // SGPR-indexed v_readlane on the chain; the VALU write of EXEC needs 4 wait states before v_readfirstlane, filled
                // with the scale * P products, the s_ff1 (lane index for the bookkeeping only) and the v_writelane (which ignores
                // EXEC; a symbol that then leaves through a trampoline is written again by its handler).  The range alternates
                // between s[52:53] (even symbols) and s[48:49] (odd): no copy of the new range; odd trampolines swap them back.
                ".p2align 6\n\t"
                "80:\n\t"
#include "ccd_dec_block16p.inc"   // one renormalisation / sentinel test per two symbols (tools/gen_decoder_block.py: block_paired)
                // ---- end of a full batch: the same hand-over as at 2: with a constant lane mask ...
                "s_mov_b64 exec, 0xffff\n\t"
                "v_sub_u32 v52, %[top], %[raw]\n\t"
                "v_add_u32 v52, 1, v52\n\t"
                "ds_write_b8 %[ring], v52\n\t"
                "global_store_byte %[goff], v52, %[lat]\n\t"
                "s_mov_b64 exec, -1\n\t"
                "ds_write_b32 v51, %[zero]\n\t"
                "s_add_u32 %[seq], %[seq], 1\n\t"
                "s_add_u32 s58, %[pix0], %[i]\n\t"
                "v_mov_b32 v56, %[seq]\n\t"
                "v_mov_b32 v57, s58\n\t"
                "ds_write_b64 %[rdy], v[56:57] offset:64\n\t"
                // ---- ... then the next batch of this step (if any): its ready counter, top symbols and first two rows are requested
                // straight into the registers the loop uses (the finished batch's are dead by now); LDS answers a wave in order
                // and producers store rows before they count a part in, so a counter that reads complete vouches for the rows
                // read after it.  The ring / latent-grid positions advance while the answers travel (a finished step leaves
                // them: the compiled code sets them per step).
                "22:\n\t"
                "s_and_b32 s55, %[seq], %[smask]\n\t"
                "v_lshl_add_u32 v51, s55, 2, %[rdy]\n\t"
                "ds_read_b32 v54, v51\n\t"
                "s_lshl_b32 s56, s55, %[bshift]\n\t"
                "v_lshl_add_u32 v53, s56, 2, %[l4]\n\t"
                "ds_read_b32 %[top], v53\n\t"
                "ds_read_b32 %[ring], v53 offset:520\n\t"
                "ds_read_b32 %[goff], v53 offset:1040\n\t"
                "v_lshl_add_u32 v50, s56, 9, %[tabl]\n\t"
                "ds_read2st64_b64 v[40:43], v50 offset1:1\n\t"
                // a FULL batch of this step ahead (the common case on the wide grids): its end index needs no clamp, its ready word
                // is compared with the constant "all parts", and nothing else is tested (s72 = n on grids with 16-symbol batches,
                // 0 on the others: never full)
                "s_add_u32 s54, %[i], s69\n\t"
                "s_cmp_le_u32 s54, s72\n\t"
                "s_cbranch_scc0 25f\n\t"
                "s_waitcnt lgkmcnt(4)\n\t"          // the counter (the first of the five answers)
                "v_readfirstlane_b32 s59, v54\n\t"
                "s_cmp_eq_u32 s59, s73\n\t"
                "s_cbranch_scc1 80b\n\t"
                "s_mov_b32 s57, s73\n\t"
                "s_branch 23f\n\t"
                "25:\n\t"
                "s_cmp_lt_u32 %[i], %[n]\n\t"
                "s_cbranch_scc0 30f\n\t"
                "s_add_u32 s54, %[i], s69\n\t"
                "s_min_u32 s54, s54, %[n]\n\t"
                "24:\n\t"
                "s_sub_u32 s58, s54, %[i]\n\t"
                "s_add_u32 s57, s58, s70\n\t"
                "s_lshr_b32 s57, s57, %[tshift]\n\t"
                "s_bfm_b32 s57, s57, 0\n\t"
                "s_waitcnt lgkmcnt(4)\n\t"          // the counter (the first of the five answers)
                "v_readfirstlane_b32 s59, v54\n\t"
                "s_cmp_eq_u32 s59, s57\n\t"
                "s_cbranch_scc0 23f\n\t"
                "s_cmp_eq_u32 s58, 16\n\t"
                "s_cbranch_scc1 80b\n\t"
                "s_branch 31b\n\t"
                // not complete when asked: poll it like a batch entered from the top (v51 = its counter, v53 = its top symbols)
                "23:\n\t"
                "s_mov_b32 s68, 0\n\t"
                "s_branch 11b\n\t"
                // ---- the step is finished.  The next one (x + 10 y = c + 1) starts one pixel to the right in the same row, or - past
                // the right edge - at x = W - 10 one row down; its first batch sits in the slot just requested.  Everything the
                // compiled code derives per step (StepIter, lane positions) is advanced here: ~25 instructions instead of ~90
                // and two region crossings per step (there are W + 10 (H - 1) steps per grid).  Restates StepWalk::next of
                // ccd_wavefront.hpp in assembly, with its multiply-shift for x0 / 10.
                "30:\n\t"
                "s_add_u32 %[pix0], %[pix0], %[n]\n\t"
                "s_sub_u32 %[cleft], %[cleft], 1\n\t"
                "s_cmp_eq_u32 %[cleft], 0\n\t"
                "s_cbranch_scc1 10f\n\t"
                "s_add_u32 %[x0], %[x0], 1\n\t"
                "s_cmp_eq_u32 %[x0], %[gw]\n\t"
                "s_cselect_b32 %[x0], s64, %[x0]\n\t"
                "s_cselect_b32 s60, 1, 0\n\t"
                "s_sub_u32 %[hy], %[hy], s60\n\t"     // rows left below the step's first
                "s_mul_i32 s60, %[x0], 0xcccd\n\t"    // x0 / 10 (wf_div10)
                "s_lshr_b32 s60, s60, 19\n\t"
                "s_add_u32 s60, s60, 1\n\t"
                "s_min_u32 %[n], s60, %[hy]\n\t"
                "s_mul_i32 s72, %[n], s61\n\t"
                "s_mov_b32 %[i], 0\n\t"
                "s_min_u32 s54, s69, %[n]\n\t"
                "s_branch 24b\n\t"
                "10:\n\t"
                "s_mov_b32 %[st], 0\n\t"
                "s_branch 4f\n\t"
#include "ccd_dec_tramp16p.inc"
                // ---- the two 8-symbol parts of a batch that is decoded part by part (the producers are the limit: every short-step
                // grid, grid 0 of a portrait picture): the paired block above cut in two, each half ending in the part-end handler 2:
#include "ccd_dec_parts8.inc"
#include "ccd_dec_parts4.inc"     // chained 4-symbol parts (r06; unchained, each through the part-end handler: 0.2 % slower)
                "15:\n\t"
                "s_mov_b32 %[st], 3\n\t"
                "s_branch 4f\n\t"
                "14:\n\t"
                "s_mov_b32 %[st], 1\n\t"
                "4:\n\t"
                "s_mov_b32 %[kr], s44\n\t"
                "s_mov_b64 %[dst], s[50:51]\n\t"
                "s_mov_b64 %[rng], s[52:53]\n\t"
                "s_waitcnt lgkmcnt(0)\n\t"
                : [dst] "+s"(rc_dist), [rng] "+s"(rc_range), [i] "+s"(i), [seq] "+s"(seq), [raw] "+v"(raw), [top] "+v"(top_l),
                  [ring] "+v"(v_ring), [goff] "+v"(v_goff), [spins] "+s"(n_spins), [wpos] "+s"(word_pos), [st] "=s"(status), [kr] "=s"(k_rare),
                  [n] "+s"(n_step), [x0] "+s"(step_x0), [hy] "+s"(step_hy), [cleft] "+s"(steps_left),
                  [pix0] "+s"(pix0), [npart] "+s"(n_part)
                : [mode] "s"(mode), [gw] "s"(static_cast<uint32_t>(grid_w)), [smask] "s"(static_cast<uint32_t>(slot_mask)),
                  [bshift] "s"(bpx_shift), [tshift] "s"(static_cast<uint32_t>(task_shift)),
                  [rdy] "v"(ready_base), [zero] "v"(0u),
                  [wbuf] "v"(wbuf), [wbase] "s"(wbase), [tabl] "v"(tab_lane), [lane] "v"(static_cast<uint32_t>(lane)),
                  [l4] "v"(lane_top_off), [lat] "s"(lat_addr)
                : "memory", "vcc", "scc", "m0", "s40", "s41", "s42", "s43", "s44", "s46", "s47", "s48", "s49", "s50", "s51", "s52", "s53", "s54", "s55",
                  "s56", "s57", "s58", "s59", "s60", "s61", "s62", "s63", "s64", "s65", "s66", "s67", "s68", "s69", "s70", "s71", "s72", "s73", "s74", "s75", "s76", "s77", "s78", "s79", "s80", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61");
#pragma clang diagnostic pop
            if (status == 0) break;  // every step of the segment is done
            if (status == 3) {  // the region renormalised with the last buffered payload word: refill, resume inside the batch
                wbase = word_pos;
                wbuf = (wbase + lane < n_words) ? words_g[wbase + lane] : 0u;
                mode = 1;
                continue;
            }
            // first symbol of the batch that holds symbol i (status 2 leaves in front of a part of it, status 1 in front of symbol i)
            const int i0 = static_cast<int>(i & ~static_cast<uint32_t>(bpx - 1));
            const int slot = uni(static_cast<int>(seq) & slot_mask);
            const int row0 = slot * bpx;
            if (status == 2) {  // the batch starting at symbol i is not complete yet: poll, then enter again
                const int cnt = min(bpx, static_cast<int>(n_step) - i0);
                const uint32_t n_parts = static_cast<uint32_t>((cnt + task_pix - 1) >> task_shift);
#ifdef CCD_PIPE_PROFILE
                const unsigned long long ts = __builtin_amdgcn_s_memtime();
#endif
                if (!wait_ge(&C.s_ready[slot], (1u << n_parts) - 1u, C.s_abort)) { ok = false; break; }  // one bit per part, all of them
#ifdef CCD_PIPE_PROFILE
                const unsigned long long dts = __builtin_amdgcn_s_memtime() - ts;
                S.stall_ticks += dts;
                S.stall_events += 1;
                if (n_step >= 48) S.wait_by_j[min(i0 / bpx, 5)] += dts;  // finest grid: stall ticks by batch position
#endif
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                mode = (i & static_cast<uint32_t>(bpx - 1)) ? 1u : 0u;  // inside a batch: re-entry behind symbol i - 1
                continue;
            }
            S.n_rare += 1;  // (always counted: status[62]; a few per stream)
            // ---- rare path for symbol i (state untouched by the asm region) -----------------------------------
            const int pi = static_cast<int>(i) - i0;  // pixel within the batch
            const uint2* tab = C.s_tab + static_cast<size_t>(row0) * 64 + lane;
            const uint2 cur = tab[pi * 64];
            const uint32_t sc_lo = static_cast<uint32_t>(rc_range >> 24);
            const uint32_t sc_hi = static_cast<uint32_t>(rc_range >> 56);
            const uint64_t p0 = static_cast<uint64_t>(sc_lo) * cur.x;
            const uint32_t p_lo = static_cast<uint32_t>(p0);
            const uint32_t p_hi = static_cast<uint32_t>(p0 >> 32) + __umul24(sc_hi, cur.x);
            int k = static_cast<int>(k_rare);
            const uint32_t l_lo = static_cast<uint32_t>(__builtin_amdgcn_readlane(p_lo, k));
            const uint32_t l_hi = static_cast<uint32_t>(__builtin_amdgcn_readlane(p_hi, k));
            const uint32_t psel = static_cast<uint32_t>(__builtin_amdgcn_readlane(cur.y, k));
            uint64_t nd = rc_dist - ((static_cast<uint64_t>(l_hi) << 32) | l_lo);
            uint64_t nr = static_cast<uint64_t>(sc_lo) * psel + (static_cast<uint64_t>(sc_hi * psel) << 32);
            if (nr == 0) {
                S.n_search += 1;  // status[63]
                // symbol outside the window (or invalid data): full 128-way search
                const uint64_t scale = rc_range >> kRcPrecision;
                if ((rc_dist >> kRcPrecision) >= scale) {
                    lds_write_release(C.s_abort, static_cast<uint32_t>(-CCD_ERR_INVALID_DATA));
                    ok = false;
                    break;
                }
                const double mu = -64.0 + static_cast<double>(meta.mu_idx[row0 + pi]) * (1.0 / 256.0);
                const double rcp = meta.rcp[row0 + pi];
                const uint32_t f0 = window_left(mu, rcp, kAcLo + lane, C.s_exp);
                const uint32_t f1 = window_left(mu, rcp, kAcLo + 64 + lane, C.s_exp);
                const unsigned long long m0 = __ballot(scale * f0 <= rc_dist), m1 = __ballot(scale * f1 <= rc_dist);
                const int sidx = __popcll(m0) + __popcll(m1) - 1;
                const uint32_t left = uni(static_cast<uint32_t>(__shfl(sidx < 64 ? f0 : f1, sidx & 63)));
                uint32_t right = uni(static_cast<uint32_t>(__shfl(sidx + 1 < 64 ? f0 : f1, (sidx + 1) & 63)));
                if (sidx == kAlphabet - 1) right = 1u << kRcPrecision;
                nd = rc_dist - scale * left;
                nr = scale * static_cast<uint64_t>(right - left);
                k = uni(1 - ((sidx + kAcLo) - meta.top[row0 + pi]));  // top - (k - 1) == symbol
            }
            if (static_cast<uint32_t>(nr >> 32) == 0) {
                nr <<= 32;
                nd = (nd << 32) | static_cast<uint32_t>(__builtin_amdgcn_readlane(wbuf, (word_pos - wbase) & 63));
                ++word_pos;
                if (word_pos - wbase == 64) { wbase = word_pos; wbuf = (wbase + lane < n_words) ? words_g[wbase + lane] : 0u; }
            }
            rc_dist = uni(nd); rc_range = uni(nr);
            asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(raw) : "s"(k), "s"(pi));
            ++i;
            mode = 1;
        }
    }
    S.dist = rc_dist; S.range = rc_range; S.word_pos = word_pos; S.wbase = wbase; S.wbuf = wbuf;
    S.n_spins += n_spins;
    S.n_part_batches += n_part;
    return seq;
}

// =================================================================================================
// PRODUCERS (waves 1..): one grid.  NV = in_pad / 4.
// =================================================================================================
// One v_mad_i64_i32 per multiply-add.  The empty asm pins every partial sum: without it the optimiser re-associates
// the wrapping int64 sums into one long dependent chain per output and expands part of the products into 64 x 64
// multiplies (an asm statement holding the instruction itself makes the hazard recogniser pad every one with s_nop).
__device__ __forceinline__ void mad64(int64_t& acc, int32_t x, int32_t w) {
    acc += static_cast<int64_t>(x) * static_cast<int64_t>(w);
    asm("" : "+v"(acc));
}
// ReLU of a Q16 accumulator as the next layer's input, (a < 0 ? 0 : a) >> 16 in 32 bits, with the sign as an and-mask: a compare
// goes through VCC, and the select that reads VCC within two slots of the compare gets s_nop from the hazard recogniser
__device__ __forceinline__ int32_t relu_q16(int64_t a) {
    return static_cast<int32_t>(a >> 16) & ~static_cast<int32_t>(a >> 63);
}
#define CCD_MAD4(ACC, X, Wv, NCH)                                                   \
    _Pragma("unroll") for (int g_ = 0; g_ < (NCH); ++g_) mad64(ACC[g_], (X).x, Wv[g_].x); \
    _Pragma("unroll") for (int g_ = 0; g_ < (NCH); ++g_) mad64(ACC[g_], (X).y, Wv[g_].y); \
    _Pragma("unroll") for (int g_ = 0; g_ < (NCH); ++g_) mad64(ACC[g_], (X).z, Wv[g_].z); \
    _Pragma("unroll") for (int g_ = 0; g_ < (NCH); ++g_) mad64(ACC[g_], (X).w, Wv[g_].w);
// one output per lane (2-pixel tasks): a second partial sum, so that no multiply-add directly follows the one it depends on
#define CCD_MAD4_PAIR(ACC, ACC2, X, Wv)                                             \
    mad64(ACC[0], (X).x, Wv[0].x); mad64(ACC2, (X).y, Wv[0].y); mad64(ACC[0], (X).z, Wv[0].z); mad64(ACC2, (X).w, Wv[0].w);
// The late path (the layers behind the first one, the output layer) pays an issue slot for every s_nop.  The hazard recogniser
// treats the empty asm as an instruction of unknown kind that wrote the accumulator and wants one instruction between it and the
// next reader; the scheduler, free to move the asm statements, bunches them in front of a multiply-add that then gets its
// s_nop (about one per three multiply-adds, whatever the number of chains).  mad64_seq fixes the order instead: multiply-add,
// its pin, then the next chain's - with two or more chains in rotation no multiply-add stands right behind its own pin.
__device__ __forceinline__ void mad64_seq(int64_t& acc, int32_t x, int32_t w) {
    mad64(acc, x, w);
    __builtin_amdgcn_sched_barrier(0);
}
#define CCD_MAD4_SEQ(ACC, X, Wv, NCH)                                               \
    _Pragma("unroll") for (int g_ = 0; g_ < (NCH); ++g_) mad64_seq(ACC[g_], (X).x, Wv[g_].x); \
    _Pragma("unroll") for (int g_ = 0; g_ < (NCH); ++g_) mad64_seq(ACC[g_], (X).y, Wv[g_].y); \
    _Pragma("unroll") for (int g_ = 0; g_ < (NCH); ++g_) mad64_seq(ACC[g_], (X).z, Wv[g_].z); \
    _Pragma("unroll") for (int g_ = 0; g_ < (NCH); ++g_) mad64_seq(ACC[g_], (X).w, Wv[g_].w);
#define CCD_MAD4_PAIR_SEQ(ACC, ACC2, X, Wv)                                         \
    mad64_seq(ACC[0], (X).x, Wv[0].x); mad64_seq(ACC2, (X).y, Wv[0].y); mad64_seq(ACC[0], (X).z, Wv[0].z); mad64_seq(ACC2, (X).w, Wv[0].w);

// ---- the ARM on the matrix cores (MF = true) ---------------------------------------------------------------------------
// v_mfma_i32_16x16x64_i8 with N = the (<= 16) pixels of a task, M = output neurons, K = (input, signed-digit byte):
// every operand is split into signed bytes (x = sum d_j 256^j, d_j in [-128, 127]: the bytes of (x + 0x808080) ^ 0x808080),
// byte products with i + j = s accumulate in one i32 tile (|partial| < 2^21) and the tiles are recombined with 64-bit
// shift-adds, so the result is the int64 sum of armint.py:180-203 exactly.  Lane l = 16 g + n holds pixel n; the accumulator
// of rows 4 g + r lands in lane group g, register r - which is where the next layer's B operand wants it when tile 1 puts
// neurons 16..19 at rows 0, 4, 8, 12: no cross-lane movement between layers.  Envelope (host: ccd_batch_plan.cpp): `narrow`
// and a worst-case IFCE feature <= 0x7F7F (two signed digits end there, not at 2^15 - 1), dim <= 20, <= 8 IFCE features,
// |weight| <= 0x7F7F7F (three signed digits end there, not at 2^23 - 1).  Hidden activations travel as three digits; a task
// that meets one above 0x7F7F7F (127.5 in Q16; no real stream has one - the crafted networks of tests/arm_envelope.py do,
// test_matrix_core_cases; EntropyParams::mfma holds an exponent so that tests can lower the limit further) is redone
// by mf_exact_task in plain int64.  tools/ubench/arm_mfma.hip is the stand-alone version of this scheme.
typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr long long kMfMaxDigits3 = 0x7F7F7F;  // largest value of three signed-digit bytes (the smallest is -0x808080)
constexpr long long kMfMaxDigits2 = 0x7F7F;    // of two
constexpr int kMfLayer1 = 8;    // A operands of the first layer: 2 tiles x 4 byte sums (tile 1 also holds the stabiliser rows 1, 2)
constexpr int kMfHidden = 10;   // per further hidden layer: 2 tiles x 5 byte sums
constexpr int kMfOut = 5;       // output layer: rows 0 (mu), 1 (log-scale)
__host__ __device__ constexpr int mf_tables(int n_layers) { return kMfLayer1 + (n_layers - 2) * kMfHidden + kMfOut; }

__device__ __forceinline__ uint32_t mf_byte(int32_t w, int j) {  // signed digit j of w as a byte (0 outside 0..2)
    const uint32_t d = (static_cast<uint32_t>(w) + 0x00808080u) ^ 0x00808080u;
    return (j < 0 || j > 2) ? 0u : ((d >> (8 * j)) & 0xffu);
}
// Which input the K-slot (lane group g, byte beta) of a layer carries and which of its bytes; -1: none.
// First layer: spatial context k = g + 4 t at byte t (one byte), IFCE feature f = g + 4 u at bytes 8 + 2 u, 9 + 2 u.
// Later layers: activations 4 g + a (a < 4: tile 0, registers 0..3) and 16 + g (a = 4: tile 1, register 0), 3 bytes each.
__device__ __forceinline__ int mf_slot_input(bool first, int g, int beta, int n_sp, int n_if, int dim, int* limb) {
    if (first) {
        if (beta < 8) { *limb = 0; const int k = g + 4 * beta; return k < n_sp ? k : -1; }
        if (beta < 12) { *limb = (beta - 8) & 1; const int f = g + 4 * ((beta - 8) >> 1); return f < n_if ? n_sp + f : -1; }
        return -1;
    }
    if (beta >= 15) return -1;
    const int a = beta / 3;
    *limb = beta - 3 * a;
    const int k = a < 4 ? 4 * g + a : 16 + g;
    return k < dim ? k : -1;
}
// 5 activations -> 15 signed-digit bytes in 4 dwords (byte 15 = 0)
__device__ __forceinline__ i32x4 mf_pack15(const int32_t (&a)[5]) {
    uint32_t d[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) d[i] = ((static_cast<uint32_t>(a[i]) + 0x00808080u) ^ 0x00808080u) & 0x00ffffffu;
    i32x4 r;
    r[0] = static_cast<int>(d[0] | (d[1] << 24));
    r[1] = static_cast<int>((d[1] >> 8) | (d[2] << 16));
    r[2] = static_cast<int>((d[2] >> 16) | (d[3] << 8));
    r[3] = static_cast<int>(d[4]);
    return r;
}
// bias + (sum_s c_s 256^s) 2^16: first layer (its inputs are the raw values, armint.py:193 shifts them by 16)
__device__ __forceinline__ int64_t mf_comb4(const i32x4 (&c)[4], int r, int64_t bias) {
    const int32_t lo = c[0][r] + (c[1][r] << 8), hi = c[2][r] + (c[3][r] << 8);
    return bias + (static_cast<int64_t>(lo) << 16) + (static_cast<int64_t>(hi) << 32);
}
// bias + sum_s c_s 256^s: later layers (Q16 activations)
__device__ __forceinline__ int64_t mf_comb5(const i32x4 (&c)[5], int r, int64_t bias) {
    const int32_t lo = c[0][r] + (c[1][r] << 8), mid = c[2][r] + (c[3][r] << 8);
    return bias + lo + (static_cast<int64_t>(mid) << 16) + (static_cast<int64_t>(c[4][r]) << 32);
}

// A operands [mf_tables][64 lanes] x 16 bytes from the staged int32 weights (whole workgroup, once per stream).
__device__ void mf_build_tables(const PipeCtx& C, int in_pad, uint32_t* s_a_words, int tid) {
    const int dim = C.dim, n_layers = C.n_layers, n_sp = C.n_sp, n_if = C.n_if;
    const int n_tab = mf_tables(n_layers);
    for (int e = tid; e < n_tab * 256; e += kPipeThreads) {
        const int idx = e >> 8, ln = (e >> 2) & 63, dw = e & 3, m = ln & 15, g = ln >> 4;
        int layer, tile, s;
        if (idx < kMfLayer1) { layer = 0; tile = idx >> 2; s = idx & 3; }
        else {
            const int j = idx - kMfLayer1, hl = j / kMfHidden;
            if (hl < n_layers - 2) { layer = 1 + hl; tile = (j - hl * kMfHidden) / 5; s = (j - hl * kMfHidden) % 5; }
            else { layer = n_layers - 1; tile = 0; s = j - (n_layers - 2) * kMfHidden; }
        }
        const int32_t* row = nullptr;  // Wt[out][.] of the output this row computes
        if (layer == n_layers - 1) { if (m < 2) row = C.s_w + C.n_w_hidden + m * in_pad; }
        else {
            int o = -1;
            if (tile == 0) o = m;
            else if ((m & 3) == 0) o = 16 + (m >> 2);
            if (o >= 0 && o < dim) row = C.s_w + layer * dim * in_pad + o * in_pad;
            if (layer == 0 && tile == 1 && (m == 1 || m == 2)) row = C.s_w + C.n_w_hidden + 2 * in_pad + (m - 1) * in_pad;  // stabiliser
        }
        uint32_t word = 0;
        if (row)
            for (int bb = 0; bb < 4; ++bb) {
                int limb = 0;
                const int k = mf_slot_input(layer == 0, g, dw * 4 + bb, n_sp, n_if, dim, &limb);
                if (k >= 0) word |= mf_byte(row[k], s - limb) << (8 * bb);
            }
        s_a_words[e] = word;
    }
}

// The task in plain int64 (rare: an activation left the 3-byte range).  Lanes 0..cnt-1 each run their pixel's whole MLP
// through two private rows of the wave's LDS tile [16][in_pad]; returns the two table indices like the fast path.
template <int NV>
__device__ __forceinline__ void mf_exact_task(const PipeCtx& C, int32_t* tile, int n, int y, int x, int W, int fin, int fw, int feat_plane,
                                              int ring_mask, int64_t& out_mu, int64_t& out_ls) {
    constexpr int in_pad = 4 * NV;
    const EntropyParams& P = *C.P;
    const int dim = C.dim, n_layers = C.n_layers, n_sp = C.n_sp;
    int32_t* ain = tile + n * in_pad;
    int32_t* aout = tile + (8 + n) * in_pad;
#pragma unroll 1
    for (int k = 0; k < dim; ++k) {
        int32_t v = 0;
        if (k < n_sp) {
            const int yy = y - P.ctx_dy[k], xx = x + P.ctx_dx[k];
            if (yy >= 0 && xx >= 0 && xx < W) v = C.s_ring[ring_cell(yy, xx, ring_mask)];
        } else if (fin > 0) {
            v = reinterpret_cast<const int16_t*>(P.ifce_feat)[((y >> 1) * fw + (x >> 1)) * C.fstride + (k - n_sp)];
        }
        ain[k] = v << 16;
    }
    int64_t stab[2];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        int64_t acc = C.s_b[(n_layers - 1) * dim + 2 + o];
        const int32_t* w = C.s_w + C.n_w_hidden + 2 * in_pad + o * in_pad;
#pragma unroll 1
        for (int k = 0; k < dim; ++k) acc += static_cast<int64_t>(ain[k]) * w[k];
        stab[o] = acc;
    }
#pragma unroll 1
    for (int l = 0; l < n_layers - 1; ++l) {
#pragma unroll 1
        for (int o = 0; o < dim; ++o) {
            int64_t acc = C.s_b[l * dim + o];
            const int32_t* w = C.s_w + l * dim * in_pad + o * in_pad;
#pragma unroll 1
            for (int k = 0; k < dim; ++k) acc += static_cast<int64_t>(ain[k]) * w[k];
            aout[o] = static_cast<int32_t>((acc < 0 ? 0 : acc) >> 16);
        }
        int32_t* t = ain; ain = aout; aout = t;
    }
#pragma unroll
    for (int o = 0; o < 2; ++o) {
        int64_t acc = C.s_b[(n_layers - 1) * dim + o] + stab[o];
        const int32_t* w = C.s_w + C.n_w_hidden + o * in_pad;
#pragma unroll 1
        for (int k = 0; k < dim; ++k) acc += static_cast<int64_t>(ain[k]) * w[k];
        if (o == 0) out_mu = acc; else out_ls = acc;
    }
}

// ---- exactness of the 32-bit operands --------------------------------------------------------------------------------
// The reference's ARM is wrapping int64 for any weights and data (armint.py:180-203).  The producers below multiply
// int32 x int32 -> int64 (v_mad_i64_i32) and sum in wrapping int64: the same numbers whenever every OPERAND is exact in
// 32 bits.  Decided on the host from the weights alone (ccd_format.cpp; else the slot runs ccd_entropy.hip): every weight
// fits int32, and no hidden activation can leave int32 even for worst-case inputs (every network seen so far has a margin
// of >= 2^3 there).  Latents << 16: always exact.  IFCE features << 16 depend on the data - the worst case of a real
// network exceeds 2^15 (three of the six networks the reference encoder produced in the build container), its features
// reach ~2^10: a feature with |f| >= 2^feat_bits is a sentinel in the int16 plane and its value sits in the int32 side
// plane; a task learns of a sentinel when it loads its features, before it waits for anything, and a pixel that met one
// is redone here in plain 64 x 64 -> 64 arithmetic.  No stream of the reference encoder takes it; the crafted networks of
// tests/arm_envelope.py do at the default limit (feat_dyn, feat_side_plane, ifce_w_*: test_every_case_on_the_production_path),
// and tests lower feat_bits to drive ordinary streams through it (EntropyParams::feat_bits).
constexpr int16_t kFeatSentinel = -32768;

// One pixel's ARM in plain wrapping int64, the whole wave on it: lane k holds input / activation k (dim <= 32), lane o
// computes output o of a layer with the activations broadcast one by one.  Every context of the pixel is decoded by now
// (the caller is past the late wait).  Returns the two output sums (before >> 24) to every lane.  (As a real call it cost
// the kernel 208 bytes of scratch per lane and the decoder its scalar operands; inlined it costs nothing outside its branch.)
struct ExactArgs {
    const EntropyParams* P;
    uint32_t s_w, s_b, s_ring;  // LDS byte offsets
    int n_w_hidden, dim, n_layers, n_sp, in_pad;
    int W, fin, fw, feat_plane, ring_mask, fstride;
};
struct ExactOut { int64_t mu, ls; };
__device__ __forceinline__ ExactOut exact_pixel(const ExactArgs& A, int y, int x) {
    const EntropyParams& P = *A.P;
    const int lane = threadIdx.x & 63;
    const int dim = A.dim, n_layers = A.n_layers, n_sp = A.n_sp, in_pad = A.in_pad;
    const int32_t* s_w = reinterpret_cast<const int32_t*>(ccd_pipe_smem + A.s_w);
    const int64_t* s_b = reinterpret_cast<const int64_t*>(ccd_pipe_smem + A.s_b);
    const int8_t* s_ring = reinterpret_cast<const int8_t*>(ccd_pipe_smem + A.s_ring);
    uint64_t xin = 0;
    if (lane < dim) {
        int64_t v = 0;
        if (lane < n_sp) {
            const int yy = y - P.ctx_dy[lane], xx = x + P.ctx_dx[lane];
            if (yy >= 0 && xx >= 0 && xx < A.W) v = s_ring[ring_cell(yy, xx, A.ring_mask)];
        } else if (A.fin > 0) {
            const int pos = (y >> 1) * A.fw + (x >> 1);
            v = reinterpret_cast<const int16_t*>(P.ifce_feat)[pos * A.fstride + (lane - n_sp)];
            // side plane (planar): the raw Q8 sum; the reference sends it through float32 and back (coolchic.py:142-144)
            if (v == kFeatSentinel) v = static_cast<int64_t>(static_cast<float>(P.ifce_wide[(lane - n_sp) * A.feat_plane + pos]));
        }
        xin = static_cast<uint64_t>(v) << 16;  // armint.py:193
    }
    auto bcast = [&](uint64_t v, int k) {
        const uint32_t lo = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(v)), k));
        const uint32_t hi = static_cast<uint32_t>(__shfl(static_cast<int>(static_cast<uint32_t>(v >> 32)), k));
        return (static_cast<uint64_t>(hi) << 32) | lo;
    };
    // rows of Wt[out][in_pad] starting at `wt`, biases at `bias`; lanes >= n_out compute a discarded copy of the last row
    auto layer = [&](const int32_t* wt, const int64_t* bias, int n_out, uint64_t xv) {
        const int o = min(lane, n_out - 1);
        uint64_t acc = static_cast<uint64_t>(bias[o]);
#pragma unroll 1
        for (int k = 0; k < dim; ++k) acc += bcast(xv, k) * static_cast<uint64_t>(static_cast<int64_t>(wt[o * in_pad + k]));
        return acc;
    };
    const uint64_t stab = layer(s_w + A.n_w_hidden + 2 * in_pad, s_b + (n_layers - 1) * dim + 2, 2, xin);
    uint64_t xv = xin;
#pragma unroll 1
    for (int l = 0; l < n_layers - 1; ++l) {
        const int64_t a = static_cast<int64_t>(layer(s_w + l * dim * in_pad, s_b + l * dim, dim, xv));
        xv = static_cast<uint64_t>((a < 0 ? 0 : a) >> 16);
    }
    const uint64_t out = layer(s_w + A.n_w_hidden, s_b + (n_layers - 1) * dim, 2, xv) + stab;
    ExactOut r;
    r.mu = static_cast<int64_t>(bcast(out, 0));
    r.ls = static_cast<int64_t>(bcast(out, 1));
    return r;
}

// Sum of a 64-bit value over the 8 or 16 lanes of a pixel's group, in every lane of the group: pairs (quad_perm [1,0,3,2]),
// quads (quad_perm [2,3,0,1]), the other quad of the 8 (row_half_mirror), the other half of the 16 (row_mirror).  A group of 32
// lanes is two DPP rows: row_bcast:15 hands the even row's sum (its lane 15 holds it like every other) to the odd row, so the
// UPPER 16 lanes of the group end up with the whole sum and the lower 16 with their own row's.  Wrapping int64
// addition is associative and commutative: the same bits as any serial sum.  (The DPP reads are the compiler's: it keeps the
// wait states between a VALU write and a DPP read of the same register; two sums reduced side by side fill them.)
template <int CTRL>
__device__ __forceinline__ int64_t dpp_add64(int64_t v) {
    // (every lane of these permutations has a source lane: bound_ctrl only spares the destination's initialisation)
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(v), CTRL, 0xf, 0xf, true));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(v >> 32), CTRL, 0xf, 0xf, true));
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 other = {lo, hi};  // (a register pair as it stands: shifts and ors made two 64-bit additions of it)
    return v + __builtin_bit_cast(int64_t, other);
}
// the even row's lane 15 into every lane of the odd row behind it (rows 1 and 3 only: an even row adds zero)
__device__ __forceinline__ int64_t dpp_add64_row_below(int64_t v) {
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x142, 0xa, 0xf, false));
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v >> 32), 0x142, 0xa, 0xf, false));
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 other = {lo, hi};
    return v + __builtin_bit_cast(int64_t, other);
}
template <int LANES>
__device__ __forceinline__ void group_sum2(int64_t& a, int64_t& b) {
    static_assert(LANES == 8 || LANES == 16 || LANES == 32, "a pixel's lane group: part of a DPP row, a row, or two rows");
    a = dpp_add64<0xB1>(a); b = dpp_add64<0xB1>(b);
    a = dpp_add64<0x4E>(a); b = dpp_add64<0x4E>(b);
    a = dpp_add64<0x141>(a); b = dpp_add64<0x141>(b);
    if constexpr (LANES >= 16) { a = dpp_add64<0x140>(a); b = dpp_add64<0x140>(b); }
    if constexpr (LANES == 32) { a = dpp_add64_row_below(a); b = dpp_add64_row_below(b); }
}
// clamp((sum >> 24) + off, 0, hi) of an output-layer sum, in 32 bits.  sum >> 24 has 40 bits; with the high word clamped to
// +-2^22 first it fits 32 (|x| <= 2^30 + 255, |off| < 2^30) and saturates the same way: a high word outside +-2^22 puts
// sum >> 24 beyond +-2^30, past both ends of any table.
__device__ __forceinline__ int32_t table_index(int64_t sum, int32_t off, int32_t hi) {
    const int32_t h = min(max(static_cast<int32_t>(sum >> 32), -(1 << 22)), 1 << 22);
    const int32_t x = static_cast<int32_t>((static_cast<uint32_t>(h) << 8) | (static_cast<uint32_t>(sum) >> 24));
    return min(max(x + off, 0), hi);
}
static_assert(kMuOffset < (1 << 29) && kScaleOffset < (1 << 29) && kMuOffset >= 0 && kScaleOffset >= 0, "table_index: offsets");
static_assert(offsetof(RowMeta, top) - offsetof(RowMeta, mu_idx) == (kRows + 2) * 4, "a pixel's top symbol is stored (kRows + 2) words behind its mu index");

#if defined(CCD_PIPE_PROFILE)
constexpr int kProfLevel = CCD_PIPE_PROFILE;
#else
constexpr int kProfLevel = 0;
#endif
// The profile of a producer's tasks (CCD_PIPE_PROFILE 2 / 3 and the trace, see the top of the file), out of the task bodies: in
// a production build every method is empty.  Level 2: stamps a .. d and the task's end, summed into prof[0..3] (idle / early
// work / late wait / late work), prof[4] (between tasks), prof[8] (tasks).  Level 3: begin(phase) ... add / sub(counter,
// phase): prof[0] waits, [1] gather, [2] the MLP without its late wait, [3] window tables, [4..7] parts of the MLP, [8] tasks.
struct TaskClock {
    enum Phase { kWait, kGather, kMlp, kStab, kHidden, kOut, kTables, kPhases };
    unsigned long long* prof;
    bool p0;  // this wave is producer 0
    unsigned long long a = 0, b = 0, c = 0, d = 0, prev_end = 0, t[kPhases];
    __device__ __forceinline__ TaskClock(unsigned long long* prof_, int pw) : prof(prof_), p0(pw == 0) {}
    __device__ __forceinline__ unsigned long long stamp() const { return (kProfTrace || p0) ? __builtin_amdgcn_s_memtime() : 0ull; }
    __device__ __forceinline__ void task_begin() { if constexpr (kProfLevel == 2) { a = stamp(); if (p0 && prev_end) prof[4] += a - prev_end; } }
    __device__ __forceinline__ void early_wait_end() { if constexpr (kProfLevel == 2) b = stamp(); }
    __device__ __forceinline__ void late_wait_begin() { if constexpr (kProfLevel == 2) c = stamp(); }
    __device__ __forceinline__ void late_wait_end() { if constexpr (kProfLevel == 2) d = stamp(); }
    __device__ __forceinline__ void task_end(const PipeCtx& C, uint32_t W, uint32_t steps_left, uint32_t gidx, uint32_t word0, uint32_t px_ahead) {
        if constexpr (kProfLevel == 2) {
            const unsigned long long e = __builtin_amdgcn_s_memtime();
#if defined(CCD_PIPE_TRACE)
            if ((threadIdx.x & 63) == 0 && W == uni(g_trace_cfg[0]) && uni(g_trace_cfg[1]) - steps_left < 64u) {
                typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                u32x4* r = reinterpret_cast<u32x4*>(ccd_pipe_smem + C.trace_off + (gidx % kTraceTasks) * 32u);
                r[0] = u32x4{word0, static_cast<uint32_t>(a), static_cast<uint32_t>(b), static_cast<uint32_t>(c)};
                r[1] = u32x4{static_cast<uint32_t>(d), static_cast<uint32_t>(e), px_ahead, static_cast<uint32_t>(a >> 32)};
            }
#endif
            if (p0) { prof[0] += b - a; prof[1] += c - b; prof[2] += d - c; prof[3] += e - d; prof[8] += 1; prev_end = e; }
        }
    }
    __device__ __forceinline__ void begin(Phase p) { if constexpr (kProfLevel >= 3) t[p] = __builtin_amdgcn_s_memtime(); }
    __device__ __forceinline__ void add(int k, Phase p) { if constexpr (kProfLevel >= 3) prof[k] += __builtin_amdgcn_s_memtime() - t[p]; }
    __device__ __forceinline__ void sub(int k, Phase p) { if constexpr (kProfLevel >= 3) prof[k] -= __builtin_amdgcn_s_memtime() - t[p]; }
    __device__ __forceinline__ void count_task() { if constexpr (kProfLevel >= 3) prof[8] += 1; }
};
// ---- two pieces of the vector-ALU task body that compile to the same code as functions --------------------------------------
// Where the decoder puts the pixel's symbol (RowMeta::cell / goff), written right behind the early wait (`row`: kRows = dummy)
__device__ __forceinline__ void store_row_position(RowMeta& meta, int row, int y, int x, int W, int ring_mask) {
    meta.cell[row] = static_cast<uint32_t>(ring_cell(y, x, ring_mask));
    meta.goff[row] = static_cast<uint32_t>(y * W + x);
}
// The task's ready bit, behind its table stores: LDS requests of one wave are performed in order, so a relaxed or is enough (a
// release would wait for every outstanding access of the wave).  One ds_or_b32 from lane 0, operands in VGPRs; no election, no branch
__device__ __forceinline__ void publish_ready(uint32_t rdy_addr, uint32_t rdy_val) {
    asm volatile("" ::: "memory");
    unsigned long long exec_all;
    asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, 1\n\tds_or_b32 %1, %2\n\ts_mov_b64 exec, %0"
                 : "=&s"(exec_all) : "v"(rdy_addr), "v"(rdy_val) : "memory");
}
// One segment of a grid (all of it, or a ramp / the streamed body: GridSeg): the walk over its steps and tasks and, in the task
// loop, the vector-ALU task body (production) phase by phase.  MF: this grid's tasks run the ARM on the matrix cores instead
// (the branch in front of it); DYN_RING: the kernel's ring of decoded symbols has EntropyParams::ring_rows rows instead of
// kRingRows (every grid of a matrix-core kernel, whichever producer serves it).  Returns the batch number behind the segment.
// The vector-ALU body stands in the loop as it is: at the register limit, a phase moved into a function of its own compiles to
// other code (profiles/r10/extractions.txt, tools/isa_compare.py).
template <int NV, int kLpp, bool MF, bool DYN_RING, bool DYN, class SH>
__device__ __forceinline__ uint32_t producer_grid(const PipeCtx& C_run, unsigned long long* prof, const GridSeg& seg) {
    constexpr int in_pad = 4 * NV;
    static_assert(!SH::fixed || (!MF && SH::dim <= in_pad && SH::dim > in_pad - 4 && SH::n_sp >= 1 && SH::n_layers >= 2), "ShapeFix: vector-ALU path, matching width");
    // fixed shape: every region at its compile-time address (the same pipe_layout the kernel carved the LDS with)
    PipeCtx C_fix = C_run;
    if constexpr (SH::fixed) {
        constexpr PipeLayout L = pipe_layout(SH::dim, SH::n_layers, in_pad, kRingRows, 0);
        C_fix.s_ring.off = L.ring; C_fix.s_w.off = L.w; C_fix.s_b.off = L.b; C_fix.s_act.off = L.act; C_fix.s_a.off = L.a; C_fix.s_tab.off = L.tab;
        C_fix.s_meta.off = L.meta; C_fix.s_rcp.off = L.rcp; C_fix.s_exp.off = L.exp; C_fix.s_ready.off = L.ready; C_fix.s_consumed.off = L.consumed;
        C_fix.s_abort.off = L.abort; C_fix.n_w_hidden = L.n_w_hidden; C_fix.ring_mask = kRingRows - 1;
#if defined(CCD_PIPE_TRACE)
        C_fix.trace_off = L.end;
#endif
        C_fix.dim = SH::dim; C_fix.n_layers = SH::n_layers; C_fix.n_sp = SH::n_sp; C_fix.k_left = 0;
    }
    const PipeCtx& C = C_fix;
    constexpr int kTaskPix = 64 / kLpp;
    constexpr int kBpx = kTaskPix == 2 ? 8 : 16;   // pixels per decoder batch (see decoder_grid)
    constexpr int kHalves = kBpx / kTaskPix;
    constexpr int kNSlots = kRows / kBpx;
    constexpr int NOUT = (in_pad + kLpp - 1) / kLpp;  // outputs per lane in a hidden layer
    const int lane = threadIdx.x & 63;
    // Everything that steers the task loop is wave-uniform; stated with readfirstlane, the loop control, the dependency
    // arithmetic and the task filter run on the scalar unit instead of as exec-masked vector code.
    const int pw = uni(static_cast<int>(threadIdx.x >> 6) - 1);
    const EntropyParams& P = *C.P;
    const int dim = SH::fixed ? SH::dim : uni(C.dim), n_layers = SH::fixed ? SH::n_layers : uni(C.n_layers), n_sp = SH::fixed ? SH::n_sp : uni(C.n_sp);
    const int W = uni(C.W);
    const int k_left = SH::fixed ? 0 : uni(C.k_left), fin = uni(C.fin), fw = uni(C.fw);
    const uint32_t seq_base = uni(C.seq_base);
    // this wave's activation tile [kTaskPix][in_pad] (MF: [16][in_pad], the exact redo) + 4 dummy words (stores of lanes that own
    // no activation go there by address select: no exec mask, no skip branch)
    // (the tile's size is the KERNEL's - DYN_RING = its MF - not this instantiation's: since r04 the producers of one grid may be in
    // different instantiations at the same time, the 4-pixel one on a ramp while another wave is already in the 8-pixel body)
    int32_t* act = C.s_act + pw * ((DYN_RING ? 16 : 8) * in_pad + 4);
    [[maybe_unused]] int32_t* const act_dummy = act + (DYN_RING ? 16 : 8) * in_pad;
    const int px = MF ? (lane & 15) : lane / kLpp;   // pixel of the task
    const int q = MF ? (lane >> 4) : lane % kLpp;    // lane within the pixel's group (MF: K-slot group of the matrix operands)
    const int ring_mask = DYN_RING ? uni(C.ring_mask) : kRingRows - 1;
    [[maybe_unused]] const int n_if = uni(C.n_if), mf_bits = uni(P.mfma);
    const int4* act_row = reinterpret_cast<const int4*>(act + px * in_pad);
    // Per-lane constants of the gather: the lane always fetches inputs k = q + kLpp t.  Read through the parameter block
    // inside the task loop they were global loads on every task's path.
    int ctx_dy_l[NOUT], ctx_dx_l[NOUT];
#pragma unroll
    for (int t = 0; t < NOUT; ++t) {
        const int k = q + kLpp * t;
        ctx_dy_l[t] = k < n_sp ? P.ctx_dy[k] : 0;
        ctx_dx_l[t] = k < n_sp ? P.ctx_dx[k] : 0;
    }
    // this kernel keeps the features as int16 (|feature| < 2^15 under `narrow`): half the scratch traffic of the int32 planes
    const glb_ptr<const int16_t> ifce_feat = (glb_ptr<const int16_t>)reinterpret_cast<const int16_t*>(P.ifce_feat);
    const int feat_plane = uni(C.fh) * fw;
    const int fstride = SH::fixed ? feat_stride(SH::dim - SH::n_sp) : uni(C.fstride);
    // MF: the lane's context offsets (k = q + 4 t, dy << 16 | dx) and the left neighbour's weights of the lane's rows
    // (neurons 4 q .. 4 q + 3 and 16 + q, then the two stabiliser outputs)
    [[maybe_unused]] int32_t mf_dxy[8], mf_wl[7];
    if constexpr (MF) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int k = q + 4 * t;
            mf_dxy[t] = k < n_sp ? static_cast<int32_t>((static_cast<uint32_t>(P.ctx_dy[k]) << 16) | (static_cast<uint32_t>(P.ctx_dx[k]) & 0xffffu)) : 0;
        }
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            const int o = r < 4 ? 4 * q + r : 16 + q;
            int32_t w = 0;
            if (k_left >= 0) {
                if (r < 5) w = o < dim ? C.s_w[o * in_pad + k_left] : 0;
                else w = C.s_w[C.n_w_hidden + 2 * in_pad + (r - 5) * in_pad + k_left];
            }
            mf_wl[r] = w;
        }
    }
    TaskClock clk(prof, pw);
    constexpr uint32_t kTaskShift = kTaskPix == 8 ? 3 : (kTaskPix == 4 ? 2 : 1), kBpxShift = kBpx == 32 ? 5 : (kBpx == 16 ? 4 : 3), kHalvesShift = kBpxShift - kTaskShift;
    StepWalk it;
    it.init(static_cast<uint32_t>(uni(C.H)), static_cast<uint32_t>(W));
    uint32_t seq = seq_base;
    // pixels of the stream in front of this step, the previous one, the one before; rows the step start moved down in between
    uint32_t pix0 = uni(C.px_base), prev_pix0 = pix0, prev2_pix0 = pix0, prev_moved = 0;
    const uint32_t seg_first = uni(seg.first), seg_steps = uni(seg.steps);
    const bool seg_body = uni(seg.body ? 1 : 0) != 0;
    if (seg_first > 0u) {  // a segment behind the grid's first step (wavefront order): as if the steps in front of it had been walked
        it.seek_before(seg_first);
        pix0 += uni(seg.pix_before);
        prev_pix0 = pix0 - it.n;
        prev2_pix0 = prev_pix0 - (seg_first > 1u ? it.len_of(seg_first - 2u) : 0u);
        prev_moved = it.moved;
    }
    // Task t of a step (pixels t kTaskPix ..) has the global index seq0 kHalves + t and belongs to producer index % kProducers:
    // a producer visits only its own tasks (first owned one of the step, then every kProducers-th).
    uint32_t phase = static_cast<uint32_t>((static_cast<unsigned long long>(seq_base) * kHalves) % kProducers);  // (seq0 kHalves) mod kProducers
    const bool split = k_left >= 0 && W > 9 && n_layers >= 2;  // !wf_raster(W): the call changed all 23 instantiations
    const uint32_t n_steps_total = wf_n_steps(it.H, it.W);
    const uint32_t seg_end = seg_first + seg_steps;  // one past the segment's last step
    // leaves step `it` for the next one INSIDE a streamed body (wavefront order, not the last step: straight-line code, no test of
    // the grid's kind or end), with the bookkeeping of the dependencies: where the previous two steps begin in the stream
    const auto walk_on = [&]() {
        prev2_pix0 = prev_pix0; prev_pix0 = pix0; pix0 += it.n; prev_moved = it.moved;
        const uint32_t nx = it.x0 + 1u, mv = nx == it.W ? 1u : 0u;
        it.x0 = mv ? it.W - kWfSlope : nx; it.y0 += mv; it.moved = mv; --it.left;
        it.n = min(it.H - it.y0, wf_div10(it.x0) + 1u);
    };
    while (n_steps_total - it.left < seg_end && it.next()) {
        // one step of the segment - or, in a streamed body (StreamBody: its steps cut into tasks without regard to step ends), the
        // whole segment as one "step" of seg.n_pix pixels, during which `it` follows the tasks through the body's steps
        const uint32_t seg_n = seg_body ? uni(seg.n_pix) : it.n;
        const uint32_t seg_pix0 = pix0;
        const uint32_t nb = (seg_n + kBpx - 1) >> kBpxShift;
        const uint32_t n_tasks = (seg_n + kTaskPix - 1) >> kTaskShift;
        const uint32_t seq0 = seq;
        uint32_t t_first = static_cast<uint32_t>(pw) - phase;
        t_first += static_cast<int32_t>(t_first) < 0 ? kProducers : 0;
        {   // the task: its position, then its body (matrix cores or vector ALU), then the shared tail
            for (uint32_t task = t_first; task < n_tasks; task += kProducers) {
                const uint32_t j = task >> kHalvesShift;
                const int half = static_cast<int>(task & (kHalves - 1));
                seq = seq0 + j;
                const int slot = static_cast<int>(seq & (kNSlots - 1));
                const int i0 = static_cast<int>(task << kTaskShift);   // first pixel of the task within the segment
                const int cnt = min(kTaskPix, static_cast<int>(seg_n) - i0);
                // Where the task's pixels are: `n_a` of them in step `it` from index `ia` on, the others (streamed body only) at the
                // head of the step behind it.  The same lines serve a step-aligned segment: there `it` is the segment, the loop never
                // runs, ia = i0 and n_a = cnt - no test of the segment's kind on the path between two tasks.
                while (seg_pix0 + static_cast<uint32_t>(i0) >= pix0 + it.n) walk_on();
                const uint32_t ia = seg_pix0 + static_cast<uint32_t>(i0) - pix0;
                const uint32_t n_a = min(static_cast<uint32_t>(cnt), it.n - ia);
                const uint32_t bx1 = it.x0 + 1u, b_moved = bx1 == static_cast<uint32_t>(W) ? 1u : 0u;
                const uint32_t bx0 = b_moved ? static_cast<uint32_t>(W) - kWfSlope : bx1, by0 = it.y0 + b_moved;
                const bool in_b = static_cast<uint32_t>(px) >= n_a;  // (also the lanes behind the task's last pixel: unused)
                const int ii = in_b ? px - static_cast<int>(n_a) : static_cast<int>(ia) + px;
                const int y = static_cast<int>(in_b ? by0 : it.y0) + ii, x = static_cast<int>(in_b ? bx0 : it.x0) - kWfSlope * ii;
                const uint32_t dy1 = it.moved, dy2 = it.moved + prev_moved;
                const uint32_t prev_n = pix0 - prev_pix0, prev2_n = prev_pix0 - prev2_pix0;
                // ---- vector-ALU body, feature request.  IFCE features do not depend on this grid: REQUEST them before waiting on the
                // decoder, use them in the gather.
                // (r04: the selects stood right behind the loads, so every task began with s_waitcnt vmcnt(0) - an L2 round trip of
                // ~700 ticks on the path between two tasks.  The raw values now stay untouched until the gather, behind the early
                // wait and the tail stores.)
                uint32_t f_raw[NOUT];  // the 16 bits as loaded (sign-extended at the gather: any operation on them is a wait)
                bool f_has[NOUT];
                if constexpr (!MF) {
                    // every lane loads, whatever the grid (no branch: at a join the compiler finishes the selects, i.e. waits): a lane
                    // without a feature - or a grid without IFCE - reads the plane's first sample and drops it
                    const int fo = (y >> 1) * fw + (x >> 1);
#pragma unroll
                    for (int t = 0; t < NOUT; ++t) {
                        const int k = q + kLpp * t;
                        f_has[t] = fin > 0 && px < cnt && k >= n_sp && k < dim;
                        f_raw[t] = reinterpret_cast<glb_ptr<const uint16_t>>(ifce_feat)[f_has[t] ? fo * fstride + (k - n_sp) : 0];
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < NOUT; ++t) { f_raw[t] = 0; f_has[t] = false; }
                }
                // dynamic operand check (see exact_pixel): a sentinel among the task's features - known at the gather, BEFORE the late
                // wait, so the critical path only carries one scalar test of this mask.
                unsigned long long bad_lanes = 0ull;
                // ---- both bodies: two waits.  Of all contexts only the left neighbour (y, x - 1) lies in the previous step (pixel i of this
                // step reads pixel i of that one, pixel i + 1 when the step start moved down a row in between); (y, x - 2) lies
                // two steps back, everything else at least five.  So the task gathers every other input, runs the stabiliser and
                // the first layer on them BEFORE the left neighbour is decoded, and only adds that one term afterwards: the
                // critical path from "symbol decoded" to "table ready" loses the gather and a third of the MLP.
                // Both waits are in pixels of the stream (the decoder publishes in decoding order: a published pixel vouches
                // for every earlier step); the first one also wants the slot's previous batch gone (table / meta rows free again).
                const uint32_t need_slot = seq >= static_cast<uint32_t>(kNSlots) ? seq - kNSlots + 1 : 0;
                // (the task's LAST pixel decides: index `last1 - 1` of step `it`, or - a task that reaches into the next step - of that one)
                const bool ends_in_b = n_a < static_cast<uint32_t>(cnt);
                const uint32_t last1 = ends_in_b ? static_cast<uint32_t>(cnt) - n_a : ia + static_cast<uint32_t>(cnt);
                const uint32_t need_px = ends_in_b ? pix0 + min(last1 + b_moved, it.n) : prev_pix0 + min(last1 + dy1, prev_n);  // ... the left neighbours
                const uint32_t need_early_px = ends_in_b ? prev_pix0 + min(last1 + b_moved + dy1, prev_n)
                                                         : prev2_pix0 + min(last1 + dy2, prev2_n);                        // ... the pixels two to the left
                // ---- vector-ALU body: what it works out before the late wait and uses behind it.  The entry's role in its window
                // (sentinel, window top) as masks / addends
                uint32_t win_left_m = 0, win_keep_m = 0, win_e0 = 0, win_e1 = 0;
                // the output layer runs on the activations the lanes hold, summed over the pixel's lanes, and the
                // pixel's lanes build its window themselves from the indices they then have.  The WINDOW LANES of a pixel are
                // all of its lanes on 8- and 4-pixel tasks and the upper 16 of its 32 on 2-pixel tasks (group_sum2); kQ0 is the
                // first of them.
                constexpr int kQ0 = kLpp == 32 ? 16 : 0;
                constexpr int kEpl = kLpp == 8 ? 2 : 1;  // window entries per lane
                const int e0 = kEpl * (q & 15);          // the lane's first entry
                int32_t idx_mu = 0, idx_sc = 0;  // the pixel's table indices, in every window lane of the pixel
                double own_rcp = 0.0;            // s_rcp[idx_sc]
                uint32_t own_ent = 0;            // where the lane's table entries go
                uint32_t mu_dst = 0, rcp_dst = 0;  // where the lane's table index and reciprocal go (RowMeta; see the role constants below)
                uint32_t rdy_addr = 0, rdy_val = 0;  // the ready bit's word and value
                unsigned narrow_mask = 0;  // matrix-core path: bit i: pixel i of the task is narrow (wave-uniform)
                unsigned long long wide_lanes = 0ull;  // both bodies: the pixels that need the wide window (ballot of their log-scale lanes / MF: a bit each)
                RowMeta& meta = *C.s_meta;
                if constexpr (MF) {
                    const int n = px, g = q;  // lane = 16 g + n: pixel n of the task, K-slot group g of the matrix operands
                    const bool live = n < cnt;
                    // ---- IFCE features (two signed bytes each) do not depend on this grid: fetch them before waiting on the decoder
                    int32_t f0 = 0, f1 = 0;
                    if (live && fin > 0) {
                        const int fo = (y >> 1) * fw + (x >> 1);
                        if (g < n_if) f0 = ifce_feat[fo * fstride + g];
                        if (g + 4 < n_if) f1 = ifce_feat[fo * fstride + g + 4];
                    }
                    clk.a = LPROF_T(pw == 0);
#if defined(CCD_PIPE_PROFILE) && CCD_PIPE_PROFILE == 2
                    if (pw == 0 && clk.prev_end) prof[4] += clk.a - clk.prev_end;
#endif
                    {
                        const unsigned long long t0 = PROF_T();
                        if (!wait_ge2(C.s_consumed, need_slot, split ? need_early_px : need_px, C.s_abort)) return seq;  // (abort / lost hand-over: the kernel stops behind this grid, the count is not used)
                        PROF_ADD(prof[0], t0);
                    }
                    clk.b = LPROF_T(pw == 0);
                    const unsigned long long t_g = PROF_T();
                    {   // where the decoder puts the pixel's symbol (RowMeta::cell / goff)
                        const int mi = (g == 0 && live) ? slot * kBpx + half * kTaskPix + n : kRows;
                        meta.cell[mi] = static_cast<uint32_t>(ring_cell(y, x, ring_mask));
                        meta.goff[mi] = static_cast<uint32_t>(y * W + x);
                    }
                    // ---- B operand of the first layer: context k = g + 4 t at byte t, the two features at bytes 8..11
                    uint32_t w0 = 0, w1 = 0;
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        if (4 * t < n_sp) {
                            const int k = g + 4 * t;
                            // unconditional read of a clamped cell + select: no exec-mask branches on the task's path
                            const int yy = y - (mf_dxy[t] >> 16), xx = x + static_cast<int16_t>(mf_dxy[t] & 0xffff);
                            const bool take = live && k < n_sp && yy >= 0 && xx >= 0 && xx < W && !(split && k == k_left);
                            const int cell = take ? ring_cell(yy, xx, ring_mask) : 0;
                            int32_t v = C.s_ring[cell];
                            v = take ? v : 0;
                            if (t < 4) w0 |= static_cast<uint32_t>(v & 0xff) << (8 * t);
                            else w1 |= static_cast<uint32_t>(v & 0xff) << (8 * (t - 4));
                        }
                    }
                    const uint32_t d0 = (static_cast<uint32_t>(f0) + 0x8080u) ^ 0x8080u, d1 = (static_cast<uint32_t>(f1) + 0x8080u) ^ 0x8080u;
                    const i32x4 bop = {static_cast<int>(w0), static_cast<int>(w1), static_cast<int>((d0 & 0xffffu) | (d1 << 16)), 0};
                    PROF_ADD(prof[1], t_g);
                    const unsigned long long t_m = PROF_T();
                    const i32x4* sa = reinterpret_cast<const i32x4*>(static_cast<uint32_t*>(C.s_a)) + lane;
                    const i32x4 zero4 = {0, 0, 0, 0};
                    // ---- first layer and stabiliser on the early inputs: 2 tiles x 4 byte sums
                    int64_t pre[5], st0, st1;
                    {
                        i32x4 c1[2][4];
#pragma unroll
                        for (int t = 0; t < 2; ++t)
#pragma unroll
                            for (int s = 0; s < 4; ++s) c1[t][s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(sa[(t * 4 + s) * 64], bop, zero4, 0, 0, 0);
                        const int64_t* bl = C.s_b;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int o = 4 * g + r;
                            const int64_t bias = bl[min(o, dim - 1)];
                            pre[r] = mf_comb4(c1[0], r, o < dim ? bias : 0);
                        }
                        {
                            const int64_t bias = bl[min(16 + g, dim - 1)];
                            pre[4] = mf_comb4(c1[1], 0, 16 + g < dim ? bias : 0);
                        }
                        st0 = mf_comb4(c1[1], 1, bl[(n_layers - 1) * dim + 2]);
                        st1 = mf_comb4(c1[1], 2, bl[(n_layers - 1) * dim + 3]);
                    }
                    // A operands and biases of the next two stages: on their way before the left neighbour is waited for
                    const i32x4* sl_out = sa + (kMfLayer1 + (n_layers - 2) * kMfHidden) * 64;
                    i32x4 a_h[10], a_o[5];
                    int64_t b_h[5];
                    if (n_layers > 2) {
#pragma unroll
                        for (int s = 0; s < 10; ++s) a_h[s] = sa[(kMfLayer1 + s) * 64];
#pragma unroll
                        for (int r = 0; r < 5; ++r) {
                            const int o = r < 4 ? 4 * g + r : 16 + g;
                            const int64_t bias = C.s_b[dim + min(o, dim - 1)];
                            b_h[r] = o < dim ? bias : 0;
                        }
                    }
#pragma unroll
                    for (int s = 0; s < 5; ++s) a_o[s] = sl_out[s * 64];
                    const int64_t b_mu = C.s_b[(n_layers - 1) * dim], b_ls = C.s_b[(n_layers - 1) * dim + 1];
                    PROF_ADD(prof[4], t_m);  // first layer
                    // ---- the left neighbour: wait for it (and for the slot), add its term as a rank-1 update
                    int32_t xleft = 0;
                    clk.c = LPROF_T(pw == 0);
                    if (split) {
                        const unsigned long long t0 = PROF_T();
                        if (!wait_ge(C.s_consumed + 1, need_px, C.s_abort)) return seq;  // (abort / lost hand-over: the kernel stops behind this grid, the count is not used)
                        PROF_ADD(prof[0], t0);
                        PROF_SUB(prof[2], t0);  // the MLP's stamps bracket this wait: take it out of them
                        PROF_ADD(prof[5], t0);  // late wait
                        if (live && x >= 1) xleft = static_cast<int32_t>(C.s_ring[ring_cell(y, x - 1, ring_mask)]) << 16;
                    }
                    clk.d = LPROF_T(pw == 0);
                    const unsigned long long t_h = PROF_T();
                    int32_t av[5];
                    uint32_t big = 0;   // OR of every hidden activation of the lane (they are >= 0)
                    uint32_t over = 0;  // OR of (activation + 0x808080): bits from 24 up <=> an activation in 0x7F7F80 .. 2^23 - 1 (or beyond)
#pragma unroll
                    for (int r = 0; r < 5; ++r) {
                        mad64(pre[r], xleft, mf_wl[r]);
                        const int64_t a = pre[r] < 0 ? 0 : pre[r];
                        av[r] = static_cast<int32_t>(a >> 16);
                        big |= static_cast<uint32_t>(av[r]); over |= static_cast<uint32_t>(av[r]) + 0x00808080u;
                    }
                    mad64(st0, xleft, mf_wl[5]);
                    mad64(st1, xleft, mf_wl[6]);
                    // ---- further hidden layers: (1 or 2) tiles x 5 byte sums each
                    for (int l = 1; l < n_layers - 1; ++l) {
                        const i32x4 b2 = mf_pack15(av);
                        i32x4 c2[5], c2b[5];
#pragma unroll
                        for (int s = 0; s < 5; ++s) c2[s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_h[s], b2, zero4, 0, 0, 0);
                        if (dim > 16) {
#pragma unroll
                            for (int s = 0; s < 5; ++s) c2b[s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_h[5 + s], b2, zero4, 0, 0, 0);
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int64_t a = mf_comb5(c2, r, b_h[r]);
                            av[r] = static_cast<int32_t>((a < 0 ? 0 : a) >> 16);
                            big |= static_cast<uint32_t>(av[r]); over |= static_cast<uint32_t>(av[r]) + 0x00808080u;
                        }
                        av[4] = 0;
                        if (dim > 16) {
                            const int64_t a = mf_comb5(c2b, 0, b_h[4]);
                            av[4] = static_cast<int32_t>((a < 0 ? 0 : a) >> 16);
                            big |= static_cast<uint32_t>(av[4]); over |= static_cast<uint32_t>(av[4]) + 0x00808080u;
                        }
                        if (l + 1 < n_layers - 1) {  // deeper networks: operands of the next hidden layer
                            const i32x4* sl = sa + (kMfLayer1 + l * kMfHidden) * 64;
#pragma unroll
                            for (int s = 0; s < 10; ++s) a_h[s] = sl[s * 64];
#pragma unroll
                            for (int r = 0; r < 5; ++r) {
                                const int o = r < 4 ? 4 * g + r : 16 + g;
                                const int64_t bias = C.s_b[(l + 1) * dim + min(o, dim - 1)];
                                b_h[r] = o < dim ? bias : 0;
                            }
                        }
                    }
                    PROF_ADD(prof[6], t_h);  // left term + further hidden layers
                    const unsigned long long t_o = PROF_T();
                    // ---- output layer: rows 0 (mu) and 1 (log-scale) land in lane group 0, next to the stabiliser
                    int64_t out_mu, out_ls;
                    {
                        const i32x4 b3 = mf_pack15(av);
                        i32x4 c3[5];
#pragma unroll
                        for (int s = 0; s < 5; ++s) c3[s] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a_o[s], b3, zero4, 0, 0, 0);
                        out_mu = mf_comb5(c3, 0, b_mu) + st0;
                        out_ls = mf_comb5(c3, 1, b_ls) + st1;
                    }
                    // an activation outside the three signed digits (above 0x7F7F7F: `over` carries into bit 24), or outside the
                    // lowered limit of a test, anywhere in the task: redo the task in plain int64
                    if (__ballot(((big >> mf_bits) | (over >> 24)) != 0u) != 0ull) {
                        if (g == 0 && live) mf_exact_task<NV>(C, act, n, y, x, W, fin, fw, feat_plane, ring_mask, out_mu, out_ls);
                        if (lane == 0) atomicAdd(reinterpret_cast<int*>(P.status) + 39, 1);  // status[39]: tasks redone (tests)
                    }
                    const int64_t m8 = (out_mu >> 24) + kMuOffset, s8 = (out_ls >> 24) + kScaleOffset;
                    const int32_t idx_mu = static_cast<int32_t>(m8 < 0 ? 0 : (m8 > kNumMu - 1 ? kNumMu - 1 : m8));
                    const int32_t idx_sc = static_cast<int32_t>(s8 < 0 ? 0 : (s8 > kNumScale - 1 ? kNumScale - 1 : s8));
                    const int mpx = slot * kBpx + half * kTaskPix + n;  // table row of the pixel
                    if (g == 0 && live) {
                        meta.mu_idx[mpx] = idx_mu;
                        meta.rcp[mpx] = C.s_rcp[idx_sc];
                    }
                    narrow_mask = static_cast<unsigned>(__ballot(g == 0 && live && idx_sc <= kNarrowMaxScale)) & 0xffffu;
                    PROF_ADD(prof[2], t_m);
                    PROF_ADD(prof[7], t_o);
#if defined(CCD_PIPE_PROFILE) && CCD_PIPE_PROFILE >= 3
                    prof[8] += 1;
#endif
                    clk.begin(TaskClock::kTables);
                } else {
                // ======================== the vector-ALU task body: early wait, gather ========================
                clk.task_begin();
                // what lane q holds of the layer in front of the output layer: its units o = q + kLpp t (the raw inputs of a network
                // without a hidden layer): the output layer's inputs
                int32_t hid[NOUT];
                clk.begin(TaskClock::kWait);
                // (the early wait includes "slot free again": true long ago whenever it is looked at - the slot was last used
                // kNSlots batches back - and it lets the table rows' tails be cleared before the late wait, see below)
                if (!wait_ge2(C.s_consumed, need_slot, split ? need_early_px : need_px, C.s_abort)) return seq;  // (abort / lost hand-over: the kernel stops behind this grid, the count is not used)
                clk.add(0, TaskClock::kWait);
                clk.early_wait_end();
                clk.begin(TaskClock::kGather);
                store_row_position(meta, (q == 0 && px < cnt) ? slot * kBpx + half * kTaskPix + px : kRows, y, x, W, ring_mask);
                // ---- entries 16..63 of the task's table rows: lower sentinels of a narrow window (P = 0).  Written now, off the
                // late path: a row that turns out wide overwrites all 64 entries later.  cnt rows x 24 16-byte stores.
                {
                    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                    const u32x4 z4 = {0u, 0u, 0u, 0u};
                    uint2* const tab0 = C.s_tab + static_cast<size_t>(slot * kBpx + half * kTaskPix) * 64;
#pragma unroll
                    for (int j = 0; j < (kTaskPix * 24 + 63) / 64; ++j) {
                        const int t = lane + 64 * j, row = t / 24, e2 = t - 24 * row;
                        uint2* const dst = row < cnt ? &tab0[row * 64 + 16 + 2 * e2] : C.s_tab + kRows * 64 + 16 + 2 * (e2 % 24);  // (dummy row)
                        *reinterpret_cast<u32x4*>(dst) = z4;
                    }
                }
                // ---- gather: lane q of the pixel's group fetches inputs k = q, q + 8, ... --------------------------
                {   // every lane, branch-free: a lane of a pixel that does not exist fills its own (unused) row of the tile, a lane
                    // without an input stores to the dummy words; the ring read is unconditional (its offsets are 0 where there is no
                    // spatial context: the cell of the pixel itself, in bounds) and selected afterwards
                    int32_t rr[NOUT];
#pragma unroll
                    for (int t = 0; t < NOUT; ++t) {
                        const int yy = y - ctx_dy_l[t], xx = x + ctx_dx_l[t];
                        rr[t] = C.s_ring[ring_cell(yy, xx, ring_mask)];
                    }
                    // (a use the compiler cannot sink the reads behind: they stay unconditional - and ALL of them are on their way
                    // before the first one is waited for; one statement per read made it wait for each in turn)
                    if constexpr (NOUT == 1) asm volatile("" : "+v"(rr[0]));
                    else if constexpr (NOUT == 2) asm volatile("" : "+v"(rr[0]), "+v"(rr[1]));
                    else if constexpr (NOUT == 3) asm volatile("" : "+v"(rr[0]), "+v"(rr[1]), "+v"(rr[2]));
                    else if constexpr (NOUT == 4) asm volatile("" : "+v"(rr[0]), "+v"(rr[1]), "+v"(rr[2]), "+v"(rr[3]));
                    else {
#pragma unroll
                        for (int t = 0; t < NOUT; ++t) asm volatile("" : "+v"(rr[t]));
                    }
                    int32_t fv[NOUT];
                    bool feat_bad = false;
#pragma unroll
                    for (int t = 0; t < NOUT; ++t) {
                        asm volatile("" : "+v"(f_raw[t]));  // (first use of the loaded value: here, not at the load)
                        fv[t] = f_has[t] ? static_cast<int32_t>(static_cast<int16_t>(f_raw[t])) : 0;
                        feat_bad |= DYN && fv[t] == kFeatSentinel;
                    }
                    if constexpr (DYN) bad_lanes = __ballot(feat_bad);
#pragma unroll
                    for (int t = 0; t < NOUT; ++t) {
                        const int k = q + kLpp * t;
                        const int yy = y - ctx_dy_l[t], xx = x + ctx_dx_l[t];
                        const int32_t v = k < n_sp ? ((yy >= 0 && xx >= 0 && xx < W && !(split && k == k_left)) ? rr[t] : 0) : fv[t];
                        int32_t* const dst = k < in_pad ? act + px * in_pad + k : act_dummy;
                        *dst = v << 16;  // armint.py:193
                        hid[t] = v << 16;
                    }
                }
                clk.add(1, TaskClock::kGather);
                clk.begin(TaskClock::kMlp);
                // ---- MLP: lane computes outputs o = q + 8 t of its pixel ------------------------------------------
                int4 xv[NV];
#pragma unroll
                for (int v = 0; v < NV; ++v) xv[v] = act_row[v];
                // Lane q owns outputs q, q + kLpp, ...: their accumulators advance in lock-step (independent chains), one
                // 16-byte weight vector per output and step; every multiply-add is a single v_mad_i64_i32.
                clk.add(4, TaskClock::kMlp);  // activation reload
                clk.begin(TaskClock::kStab);
                int64_t so[2];  // [0]: stabiliser output (lanes q < 2), [1]: scratch second chain
                const int qs = q < 2 ? q : 1;  // lanes q >= 2 compute a discarded copy of row 1
                {   // ---- stabiliser branch on the raw inputs
                    const int4* wr = reinterpret_cast<const int4*>(C.s_w + C.n_w_hidden + 2 * in_pad + qs * in_pad);
                    so[0] = C.s_b[(n_layers - 1) * dim + 2 + qs];
                    so[1] = 0;
                    // weight vectors are requested ahead of their use everywhere below: left to itself the compiler reads each
                    // one right before its multiply-adds and the task eats an LDS round trip per vector
                    int4 wv[NV];
#pragma unroll
                    for (int v = 0; v < NV; ++v) wv[v] = wr[v];
#pragma unroll
                    for (int v = 0; v < NV; ++v) {  // the two chains alternate: a dependent v_mad_i64_i32 right behind its producer costs a wait state
                        const int4 w = wv[v];
                        mad64(so[0], xv[v].x, w.x); mad64(so[1], xv[v].y, w.y); mad64(so[0], xv[v].z, w.z); mad64(so[1], xv[v].w, w.w);
                    }
                }
                clk.add(5, TaskClock::kStab);
                clk.begin(TaskClock::kHidden);
                // ---- first hidden layer on the early inputs (the only layer when the late wait does not apply is handled alike:
                // the left term is then simply zero and the gather above already took the neighbour)
                int64_t acc0[NOUT];
                [[maybe_unused]] int64_t acc0_b = 0;
                int32_t wleft[NOUT], wleft_stab = 0;
                if (n_layers >= 2) {
                    const int32_t* wl = C.s_w;
                    const int64_t* bl = C.s_b;
                    const int4* wr[NOUT];
                    const int kl = split ? k_left : 0;
#pragma unroll
                    for (int t = 0; t < NOUT; ++t) {
                        const int oc = min(q + kLpp * t, dim - 1);  // rows past the layer: a discarded copy of the last one
                        wr[t] = reinterpret_cast<const int4*>(wl + oc * in_pad);
                        acc0[t] = bl[oc];
                        wleft[t] = wl[oc * in_pad + kl];
                    }
                    wleft_stab = C.s_w[C.n_w_hidden + 2 * in_pad + qs * in_pad + kl];
                    int4 w[NOUT], wn[NOUT];
#pragma unroll
                    for (int t = 0; t < NOUT; ++t) w[t] = wr[t][0];
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        if (v + 1 < NV) {
#pragma unroll
                            for (int t = 0; t < NOUT; ++t) wn[t] = wr[t][v + 1];
                        }
                        if constexpr (NOUT == 1) { CCD_MAD4_PAIR(acc0, acc0_b, xv[v], w) } else { CCD_MAD4(acc0, xv[v], w, NOUT) }
#pragma unroll
                        for (int t = 0; t < NOUT; ++t) w[t] = wn[t];
                    }
                    if constexpr (NOUT == 1) acc0[0] += acc0_b;
                }
                // ---- the left neighbour: wait for it, add its term to the first layer and the stabiliser.  The decoder's pixel count and
                // the neighbour's ring cell are requested TOGETHER (one LDS round trip instead of two on the late path): LDS requests of a
                // wave are served in order and the decoder writes the ring before it publishes the count, so a count that has
                // reached `need_px` vouches for the cell read behind it; otherwise both are read again in the polling loop.
                // Unconditional read (cell of column -1 for x = 0: in bounds, dropped by the select), no exec mask.
                int32_t xleft = 0;
                // ---- role constants of the output tail, as VGPRs and BEFORE the late wait: where this lane's table index and reciprocal
                // go in the row meta (first window lane of the pixel: mu index and, next to it, the top symbol; second: reciprocal;
                // the dummy entry kRows for a lane that has nothing to say), and the scale index above which the second window lane
                // reports a wide window.  Left to the compiler they were SGPR-pair masks (q == 0, q == 1, live) that did not fit the
                // scalar file: spilled, and reloaded with v_readlane on the late path.
                // (an opaque copy of the lane's index in its group: what is derived from it below is worked out per task, off the late
                // path - not hoisted out of the task loop and kept, or spilled, over the whole grid)
                int qo = q;
                asm volatile("" : "+v"(qo));
                const int mpx = slot * kBpx + half * kTaskPix + px;  // table row of the pixel
                mu_dst = lds_addr(&meta.mu_idx[px < cnt && qo == kQ0 ? mpx : kRows]);
                rcp_dst = lds_addr(&meta.rcp[px < cnt && qo == kQ0 + 1 ? mpx : kRows]);
                int32_t wide_above = px < cnt && qo == kQ0 + 1 ? kNarrowMaxScale : 0x7fffffff;
                asm volatile("" : "+v"(mu_dst), "+v"(rcp_dst), "+v"(wide_above));
                // The output layer's operands of this lane.  Its two partial sums (mu row, log-scale row) start from the
                // stabiliser output and the bias in the one lane that holds that row (q = 0: mu, q = 1: log-scale) and from zero
                // everywhere else, so that the sum over the pixel's lanes takes each once; the left neighbour's stabiliser weight
                // likewise.  The output weights of the lane's units o = q + kLpp t, both rows: ZERO for a unit past the layer
                // (such a lane computes a copy of unit dim - 1 in the hidden layers; the store into the activation tile drops it).
                int64_t out_m = 0, out_l = 0;
                int32_t wl_m = 0, wl_l = 0, wo_m[NOUT], wo_l[NOUT];
                {
                    const int64_t s = so[0] + so[1] + C.s_b[(n_layers - 1) * dim + qs];
                    const int64_t keep_m = qo == 0 ? -1 : 0, keep_l = qo == 1 ? -1 : 0;
                    out_m = s & keep_m;
                    out_l = s & keep_l;
                    wl_m = wleft_stab & static_cast<int32_t>(keep_m);
                    wl_l = wleft_stab & static_cast<int32_t>(keep_l);
                    asm volatile("" : "+v"(out_m), "+v"(out_l), "+v"(wl_m), "+v"(wl_l));
                    const int32_t* const w_out = C.s_w + C.n_w_hidden;
#pragma unroll
                    for (int t = 0; t < NOUT; ++t) {
                        const int o = qo + kLpp * t, oc = min(o, in_pad - 1);
                        const int32_t keep = (o - dim) >> 31;  // all ones for a unit of the layer
                        wo_m[t] = w_out[oc] & keep;
                        wo_l[t] = w_out[in_pad + oc] & keep;
                        asm volatile("" : "+v"(wo_m[t]), "+v"(wo_l[t]));
                    }
                }
                // the ready bit's word and value: wave-uniform and known here, as VGPRs for the one ds_or_b32 behind the table stores
                rdy_addr = lds_addr(&C.s_ready[slot]);
                rdy_val = 1u << half;
                asm volatile("" : "+v"(rdy_addr), "+v"(rdy_val));
                // The pixel's window lanes build its 14-symbol window.  4- and 2-pixel tasks: window lane e builds entry e.  8-pixel
                // tasks: lane q builds entries 2 q and 2 q + 1, one after the other, and stores them as one 16-byte vector.
                // A lane whose pixel does not exist - or, on 2-pixel tasks, one of the lower 16 - stores to the dummy row (address
                // selects instead of exec-masked stores, see RowMeta).
                const int e0o = kEpl * (qo & 15);
                own_ent = lds_addr(&C.s_tab[static_cast<size_t>(px < cnt && qo >= kQ0 ? mpx : kRows) * 64 + e0o]);
                // entry 0 is the upper sentinel (P = 0, left = 2^24 - 1 when its symbol is 64), entry 1 the window's top symbol,
                // entry 15 the lower sentinel (left = 0, P = 0).  win_left_m masks the left bound of the lane's LAST entry,
                // win_keep_m the P of its FIRST one (and of entry 15 where that is the same entry)
                win_left_m = e0o + kEpl - 1 == 15 ? 0u : ~0u;
                win_keep_m = (e0o == 0 || e0o == 15) ? 0u : ~0u;
                win_e0 = e0o == 0 ? (1u << kRcPrecision) - 1u : 0u;
                win_e1 = (e0o <= 1 && e0o + kEpl > 1) ? 1u : 0u;
                asm volatile("" : "+v"(own_ent), "+v"(win_left_m), "+v"(win_keep_m), "+v"(win_e0), "+v"(win_e1));
                clk.late_wait_begin();
                if (split) {
                    clk.begin(TaskClock::kWait);
                    const uint32_t want = uni(need_px);
                    const uint32_t cell = static_cast<uint32_t>(ring_cell(y, x - 1, ring_mask));
                    uint32_t seen_v;
                    int32_t r;
                    asm volatile("ds_read_b32 %0, %2 offset:4\n\tds_read_i8 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&v"(seen_v), "=&v"(r) : "v"(C.s_consumed.off), "v"(C.s_ring.off + cell) : "memory");
                    if (__builtin_expect(static_cast<int32_t>(uni(seen_v) - want) < 0, 0)) {
                        // every look of the polling loop is the same pair: the look that succeeds brings the cell along (one LDS
                        // round trip less between "published" and the late work: on the chain of every short-step grid)
                        unsigned spins = 0;
                        do {
                            if ((++spins & 1023u) == 0) {
                                if (lds_load_acquire(C.s_abort) != 0) return seq;  // (abort / lost hand-over: the kernel stops behind this grid, the count is not used)
                                if (spins > kSpinLimit) { lds_write_release(C.s_abort, static_cast<uint32_t>(-CCD_ERR_HIP)); return seq; }
                            }
                            asm volatile("ds_read_b32 %0, %2 offset:4\n\tds_read_i8 %1, %3\n\ts_waitcnt lgkmcnt(0)"
                                         : "=&v"(seen_v), "=&v"(r) : "v"(C.s_consumed.off), "v"(C.s_ring.off + cell) : "memory");
                        } while (static_cast<int32_t>(uni(seen_v) - want) < 0);
                    }
                    clk.add(0, TaskClock::kWait);
                    clk.sub(2, TaskClock::kWait);  // the MLP's stamps bracket this wait: take it out of them
                    clk.sub(6, TaskClock::kWait);
                    xleft = (px < cnt && x >= 1) ? r << 16 : 0;
                }
                clk.late_wait_end();
                // the late path is on the chain "symbol decoded -> table ready": it goes ahead of a SIMD neighbour's early work (the
                // decoder runs at priority 3).  41.03 -> 40.84 ms on kodak24 (profiles/r04/ab_entropy_late_prio.txt)
                // (priority 2 for the first task of a step, the head of its chain: no further gain)
                __builtin_amdgcn_s_setprio(1);
                mad64(out_m, xleft, wl_m);
                mad64(out_l, xleft, wl_l);
                // A layer's activations go through the tile only when another hidden layer reads them; the layer in front of the
                // output layer stays in `hid`.
                if (n_layers >= 2) {
#pragma unroll
                    for (int t = 0; t < NOUT; ++t) {
                        mad64(acc0[t], xleft, wleft[t]);
                        hid[t] = relu_q16(acc0[t]);
                    }
                    if (n_layers > 2) {
#pragma unroll
                        for (int t = 0; t < NOUT; ++t) {
                            const int o = q + kLpp * t;
                            // a lane without a real output stores to the dummy words (address select, constant over the grid): the
                            // padding inputs dim .. in_pad - 1 of the tile keep the zeros the gather put there
                            int32_t* const dst = o < dim ? act + px * in_pad + o : act_dummy;
                            *dst = hid[t];
                        }
#pragma unroll
                        for (int v = 0; v < NV; ++v) xv[v] = act_row[v];
                    }
                }
                for (int l = 1; l < n_layers - 1; ++l) {
                    const int32_t* wl = C.s_w + l * dim * in_pad;
                    const int64_t* bl = C.s_b + l * dim;
                    int64_t acc[NOUT];
                    [[maybe_unused]] int64_t acc_b = 0;
                    const int4* wr[NOUT];
#pragma unroll
                    for (int t = 0; t < NOUT; ++t) {
                        const int oc = min(q + kLpp * t, dim - 1);  // rows past the layer: a discarded copy of the last one
                        wr[t] = reinterpret_cast<const int4*>(wl + oc * in_pad);
                        acc[t] = bl[oc];
                    }
                    int4 w[NOUT], wn[NOUT];
#pragma unroll
                    for (int t = 0; t < NOUT; ++t) w[t] = wr[t][0];
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        if (v + 1 < NV) {
#pragma unroll
                            for (int t = 0; t < NOUT; ++t) wn[t] = wr[t][v + 1];
                        }
                        if constexpr (NOUT == 1) { CCD_MAD4_PAIR_SEQ(acc, acc_b, xv[v], w) } else { CCD_MAD4_SEQ(acc, xv[v], w, NOUT) }
#pragma unroll
                        for (int t = 0; t < NOUT; ++t) w[t] = wn[t];
                    }
                    if constexpr (NOUT == 1) acc[0] += acc_b;
#pragma unroll
                    for (int t = 0; t < NOUT; ++t) {
                        hid[t] = relu_q16(acc[t]);
                        asm("" : "+v"(hid[t]));
                    }
                    if (l + 2 < n_layers) {
#pragma unroll
                        for (int t = 0; t < NOUT; ++t) {
                            const int o = q + kLpp * t;
                            // a lane without a real output stores to the dummy words (address select, constant over the grid): the
                            // padding inputs dim .. in_pad - 1 of the tile keep the zeros the gather put there
                            int32_t* const dst = o < dim ? act + px * in_pad + o : act_dummy;
                            *dst = hid[t];
                        }
#pragma unroll
                        for (int v = 0; v < NV; ++v) xv[v] = act_row[v];
                    }
                }
                clk.add(6, TaskClock::kHidden);
                clk.begin(TaskClock::kOut);
                // ---- output layer -> table indices.  From registers: the lane's units times their two output weights (two chains in
                // rotation), then the sum over the pixel's lanes - every window lane of the pixel ends up with both sums (stabiliser
                // and bias came in through the chains' start values), no trip through the activation tile
#pragma unroll
                for (int t = 0; t < NOUT; ++t) { mad64_seq(out_m, hid[t], wo_m[t]); mad64_seq(out_l, hid[t], wo_l[t]); }
                group_sum2<kLpp>(out_m, out_l);
                idx_mu = table_index(out_m, kMuOffset, kNumMu - 1);
                idx_sc = table_index(out_l, kScaleOffset, kNumScale - 1);
                own_rcp = C.s_rcp[idx_sc];  // the one LDS trip between the output layer and the first f64 multiply
                // ---- a feature of some pixel was not exact in 16 bits (tests/test_arm_envelope.py; no trained network): that pixel again,
                // in plain int64; its table parameters replace what the lines above wrote from the sentinel
                if (DYN && __builtin_expect(bad_lanes != 0ull, 0)) {
                    int n_redo = 0;
                    for (int p = 0; p < cnt; ++p) {
                        if (((bad_lanes >> (p * kLpp)) & ((1ull << kLpp) - 1ull)) == 0ull) continue;
                        // opaque copies: nothing derived from them is hoisted out of this cold block into the task loop
                        ExactArgs A;
                        A.P = C.P; A.s_w = uni(C.s_w.off); A.s_b = uni(C.s_b.off); A.s_ring = uni(C.s_ring.off);
                        A.n_w_hidden = uni(C.n_w_hidden); A.dim = dim; A.n_layers = n_layers; A.n_sp = n_sp; A.in_pad = in_pad;
                        A.W = W; A.fin = fin; A.fw = fw; A.feat_plane = feat_plane; A.ring_mask = ring_mask; A.fstride = fstride;
                        asm volatile("" : "+s"(A.P), "+s"(A.s_w), "+s"(A.s_b), "+s"(A.s_ring), "+s"(A.n_w_hidden), "+s"(A.dim), "+s"(A.n_layers));
                        asm volatile("" : "+s"(A.n_sp), "+s"(A.W), "+s"(A.fin), "+s"(A.fw), "+s"(A.feat_plane), "+s"(A.ring_mask), "+s"(A.fstride));
                        const ExactOut r = exact_pixel(A, __builtin_amdgcn_readlane(y, MF ? p : p * kLpp), __builtin_amdgcn_readlane(x, MF ? p : p * kLpp));
                        if (px == p) {  // (the window lanes write the row meta from these below)
                            idx_mu = table_index(r.mu, kMuOffset, kNumMu - 1);
                            idx_sc = table_index(r.ls, kScaleOffset, kNumScale - 1);
                            own_rcp = C.s_rcp[idx_sc];
                        }
                        ++n_redo;
                    }
                    if (lane == 0) atomicAdd(reinterpret_cast<int*>(P.status) + 39, n_redo);  // status[39]: pixels redone (tests)
                }
                // lanes (px * kLpp + kQ0 + 1) of pixels that need the wide window (scale index above kNarrowMaxScale: 0.7 % of the symbols);
                // the common path only tests the ballot for zero
                wide_lanes = __ballot(idx_sc > wide_above);
                clk.add(2, TaskClock::kMlp);
                clk.add(7, TaskClock::kOut);
                clk.count_task();
                clk.begin(TaskClock::kTables);
                }
                // ---- window tables (lanes hold symbols in DESCENDING order; entry 0 = upper sentinel, trailing entries =
                // lower sentinels, both with P = 0).  Narrow pixels (small scale): 14 real symbols, built by the pixel's window lanes
                // (matrix-core path: four pixels per pass of the wave).  Wide pixels: 62 real symbols, one pixel per pass.
                const int base = slot * kBpx + half * kTaskPix;  // first table row of the task
                uint2* tab = C.s_tab + static_cast<size_t>(base) * 64;
                if constexpr (!MF) {
                    // Static layout: every pixel gets its 14-symbol window from its own window lanes, narrow or not (99.3 % are; the
                    // row of a wide pixel is rewritten in full below) - no bit-scanning of the mask on the late path.
                    {
                        int top = ((idx_mu + 128) >> 8) - 64 + 6;  // round(mu) + 6: window = [round(mu) - 7, round(mu) + 6]
                        top = max(kAcLo + 13, min(kAcLo + kAlphabet - 1, top));
                        // the row meta is for the decoder's rare path and the wide pass: plain stores by address select (the pixel's
                        // first window lane: mu index and top symbol, the second: reciprocal), nothing on this path waits for them
                        lds_at<int32_t>(mu_dst)[0] = idx_mu;
                        lds_at<int32_t>(mu_dst)[kRows + 2] = top;
                        const double rcp256 = window_rcp256(own_rcp);
                        *lds_at<double>(rcp_dst) = own_rcp;
                        const bool at_top = top == kAcLo + kAlphabet - 1;
                        const uint32_t hi_f = at_top ? win_e0 : 0u, to_full = at_top ? win_e1 : 0u;
                        uint32_t left[kEpl];
#pragma unroll
                        for (int j = 0; j < kEpl; ++j) {
                            const int ssym = top - (e0 + j - 1);  // entry 0 -> top + 1: its left bound is the window's upper edge
                            // window_left's edge cases from integers, ahead of the f64 chain and without compares next to their selects:
                            // symbols <= -64 (and the lower sentinel) give 0; symbol 64 - entry 0 of a window that reaches symbol 63 -
                            // gives 2^24, stored as 2^24 - 1 (every stored bound must fit 24 bits, see the wide pass)
                            uint32_t lo_m = static_cast<uint32_t>((kAcLo - ssym) >> 31);
                            if (j == kEpl - 1) lo_m &= win_left_m;
                            uint32_t l = window_cum_d256(window_d256(idx_mu, ssym), rcp256, C.s_exp) + static_cast<uint32_t>(ssym - kAcLo);
                            l = min(l, (1u << kRcPrecision) - 1u);
                            if (j == 0) l |= hi_f;
                            left[j] = l & lo_m;
                            // one chain after the other: a pass is bound by the issue rate of its f64 instructions, not by their
                            // latency, and two chains side by side only hold twice the registers
                            if (j + 1 < kEpl) __builtin_amdgcn_sched_barrier(0);
                        }
                        // the entry in front of the lane's first one: the last entry of lane q - 1 (DPP row_shr:1; entry 0 does not use it)
                        const uint32_t right = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(left[kEpl - 1]), 0x111, 0xf, 0xf, false));
                        if constexpr (kEpl == 1) {
                            typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                            const u32x2 ent = {left[0], (right - left[0] + to_full) & win_keep_m};
                            *lds_at<u32x2>(own_ent) = ent;
                        } else {
                            // entry 2 q + 1 is never entry 0, entry 2 q never entry 15 or 1
                            typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                            const u32x4 ent = {left[0], (right - left[0]) & win_keep_m, left[1], (left[0] - left[1] + to_full) & win_left_m};
                            *lds_at<u32x4>(own_ent) = ent;
                        }
                    }
                }
                unsigned rest = MF ? narrow_mask : 0u;
                while (rest) {
                    // up to four narrow pixels: sub-wave u = lane >> 4 handles pixel pix[u], entry e = lane & 15.  (Both passes of an
                    // 8-pixel task as two interleaved chains per lane were tried: slower - a pass is bound by the issue rate of its
                    // f64 instructions, not by their latency.)
                    int pix[4];
                    int n_here = 0;
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        pix[u] = rest ? __builtin_ctz(rest) : -1;
                        if (rest) { rest &= rest - 1; ++n_here; }
                    }
                    const int u = lane >> 4, e = lane & 15;
                    const int mine = u == 0 ? pix[0] : (u == 1 ? pix[1] : (u == 2 ? pix[2] : pix[3]));
                    const int mi = base + (mine < 0 ? pix[0] : mine);
                    const int mu_idx = meta.mu_idx[mi];
                    int top = ((mu_idx + 128) >> 8) - 64 + 6;  // round(mu) + 6: window = [round(mu) - 7, round(mu) + 6]
                    top = max(kAcLo + 13, min(kAcLo + kAlphabet - 1, top));
                    const double mu = -64.0 + static_cast<double>(mu_idx) * (1.0 / 256.0);
                    const int ssym = top - (e - 1);  // e = 0 -> top + 1: its left bound is the window's upper edge
                    uint32_t left = min(window_left(mu, meta.rcp[mi], ssym, C.s_exp), (1u << kRcPrecision) - 1u);
                    left = e == 15 ? 0u : left;
                    // entry e - 1 of the same 16-lane row (DPP row_shr:1; entry 0 does not use it)
                    const uint32_t right = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(left), 0x111, 0xf, 0xf, false));
                    uint2 ent;
                    ent.x = left;
                    ent.y = (e == 0 || e == 15) ? 0u : ((e == 1 && ssym == kAcLo + kAlphabet - 1) ? (1u << kRcPrecision) - left : right - left);
                    if (mine >= 0) {
                        tab[mine * 64 + e] = ent;
                        if (e == 0) meta.top[mi] = top;
                    }
                    // entries 16..63 of the (up to) four rows: lower sentinels (4 rows x 24 16-byte stores); the vector-ALU path
                    // cleared them before its late wait
                    if constexpr (MF) {
                        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
                        const u32x4 z4 = {0u, 0u, 0u, 0u};
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            const int t = lane + 64 * j;          // 0..95 (lanes 32..63 idle in the second round)
                            const int ru = t >= 72 ? 3 : (t >= 48 ? 2 : (t >= 24 ? 1 : 0));
                            const int rp = ru == 0 ? pix[0] : (ru == 1 ? pix[1] : (ru == 2 ? pix[2] : pix[3]));
                            if (t < 96 && rp >= 0) *reinterpret_cast<u32x4*>(&tab[rp * 64 + 16 + 2 * (t - 24 * ru)]) = z4;
                        }
                    }
                    (void)n_here;
                }
                unsigned long long wide = MF ? static_cast<unsigned long long>(((1u << cnt) - 1u) & ~narrow_mask) : wide_lanes;
                while (wide) {
                    const int bit = __builtin_ctzll(wide);
                    wide &= wide - 1;
                    const int i = MF ? bit : bit / kLpp;  // pixel of the task
                    const int mi = base + i;
                    const int mu_idx = meta.mu_idx[mi];
                    int top = ((mu_idx + 128) >> 8) - 64 + 30;  // round(mu) + 30: window = [round(mu) - 31, round(mu) + 30]
                    top = max(kAcLo + 61, min(kAcLo + kAlphabet - 1, top));
                    const int ssym = top - (lane - 1);
                    // every stored bound must fit 24 bits (v_mad_u32_u24 in the decoder): the upper sentinel of a window that
                    // reaches symbol 63 is clamped to 2^24 - 1; a hit on it only costs a detour through the slow path
                    uint32_t left = min(window_left_d256(window_d256(mu_idx, ssym), window_rcp256(meta.rcp[mi]), ssym, C.s_exp), (1u << kRcPrecision) - 1u);
                    left = lane == 63 ? 0u : left;
                    const uint32_t right = __shfl_up(left, 1);  // lane k-1 holds symbol s+1: its left bound is our right bound
                    uint2 ent;
                    ent.x = left;
                    ent.y = (lane == 0 || lane == 63) ? 0u
                            : ((lane == 1 && ssym == kAcLo + kAlphabet - 1) ? (1u << kRcPrecision) - left : right - left);
                    tab[i * 64 + lane] = ent;
                    if (lane == 0) meta.top[mi] = top;
                }
                if constexpr (!MF) publish_ready(rdy_addr, rdy_val);
                else {
                    asm volatile("" ::: "memory");
                    if (lane == 0) __hip_atomic_fetch_or(&C.s_ready[slot], 1u << half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                __builtin_amdgcn_s_setprio(0);
                asm volatile("" ::: "memory");
                clk.add(3, TaskClock::kTables);
                clk.task_end(C, static_cast<uint32_t>(W), it.left, seq0 * kHalves + task,
                             (it.left << 12) | ((task & 15u) << 8) | (static_cast<uint32_t>(pw) << 4) | static_cast<uint32_t>(cnt), need_px - pix0);
            }
        }
        seq = seq0 + nb;
        phase = (phase + nb * kHalves) % kProducers;
        if (seg_body) {  // on to the body's last step: the lines below leave it like any step
            while (n_steps_total - it.left < seg_end) walk_on();
        }
        prev2_pix0 = prev_pix0;
        prev_pix0 = pix0;
        pix0 += it.n;
        prev_moved = it.moved;
    }
    return seq;
}

// One kernel per input width NV = ceil(dim / 4): a single instantiation keeps the register file for the variant that runs
// (all widths in one kernel cost 444 SGPR spills and VGPR scratch in every path).
// DYN: the IFCE features of this network can leave 16 bits (its worst case does, FixedArm::dyn_feat) - the feature pass stores
// sentinels + the int32 side plane and the producers carry the check and the int64 redo (exact_pixel).  Networks whose worst
// case provably fits run the DYN = false instantiation: the same kernel without that code (its mere presence in the task loop
// costs ~2 %, profiles/r03/ab_entropy_dynamic_operand_check.txt).
template <int NV, bool MF, bool DYN, class SH>
__global__ __launch_bounds__(kPipeThreads) void entropy_pipe_kernel(const EntropyParams* slots_desc) {
    const EntropyParams& P = slots_desc[blockIdx.x];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int dim = P.dim;
    constexpr int in_pad = 4 * NV;
    const int n_layers = P.n_layers;
    const int n_if = P.has_ifce ? P.n_ifce_out : 0;

    // ---- LDS carve-up (all offsets multiples of 16) ----------------------------------------------
    PipeCtx C;
    C.P = &P;
    const int ring_rows = MF ? P.ring_rows : kRingRows;
    {
        const PipeLayout L = pipe_layout(dim, n_layers, in_pad, ring_rows, MF ? mf_tables(n_layers) : 0);
        C.s_ring.off = L.ring; C.s_w.off = L.w; C.s_b.off = L.b; C.s_act.off = L.act; C.s_a.off = L.a; C.s_tab.off = L.tab;
        C.s_meta.off = L.meta; C.s_rcp.off = L.rcp; C.s_exp.off = L.exp; C.s_ready.off = L.ready; C.s_consumed.off = L.consumed;
        C.s_abort.off = L.abort; C.n_w_hidden = L.n_w_hidden;
#if defined(CCD_PIPE_TRACE)
        C.trace_off = L.end;
#endif
    }
    C.ring_mask = ring_rows - 1;
    constexpr int kActRows = MF ? 16 : 8;
    double* s_rcp = smem_at<double>(C.s_rcp.off);
    double* s_exp = smem_at<double>(C.s_exp.off);
    for (int i = tid; i < kNumScale; i += kPipeThreads) s_rcp[i] = P.rcp_table[i];
    for (int i = tid; i < kExpN; i += kPipeThreads) s_exp[i] = kExpTab[i];
    C.dim = dim; C.n_layers = n_layers; C.n_sp = P.n_spatial; C.n_if = n_if;
    C.fstride = feat_stride(n_if);
    C.k_left = -1;
    for (int k = 0; k < P.n_spatial; ++k) if (P.ctx_dy[k] == 0 && P.ctx_dx[k] == -1) C.k_left = k;

    // ---- stage the network: int64 blob (w[in][out], b[out] per layer; ws[dim][2], bs[2]) -> int32 Wt[out][in_pad]
    {
        const int64_t* src = P.arm;
        for (int l = 0; l < n_layers; ++l) {
            const int n_out = (l == n_layers - 1) ? 2 : dim;
            int32_t* wt = C.s_w + (l < n_layers - 1 ? l * dim * in_pad : C.n_w_hidden);
            for (int i = tid; i < n_out * in_pad; i += kPipeThreads) {
                const int o = i / in_pad, k = i - o * in_pad;
                wt[i] = k < dim ? static_cast<int32_t>(src[k * n_out + o]) : 0;
            }
            int64_t* bb = C.s_b + (l < n_layers - 1 ? l * dim : (n_layers - 1) * dim);
            for (int i = tid; i < n_out; i += kPipeThreads) bb[i] = src[dim * n_out + i];
            src += dim * n_out + n_out;
        }
        int32_t* wst = C.s_w + C.n_w_hidden + 2 * in_pad;
        for (int i = tid; i < 2 * in_pad; i += kPipeThreads) {
            const int o = i / in_pad, k = i - o * in_pad;
            wst[i] = k < dim ? static_cast<int32_t>(src[k * 2 + o]) : 0;
        }
        if (tid < 2) C.s_b[(n_layers - 1) * dim + 2 + tid] = src[dim * 2 + tid];
    }
    for (int i = tid; i < kProducers * (kActRows * in_pad + 4); i += kPipeThreads) C.s_act[i] = 0;
    if constexpr (MF) {
        __syncthreads();  // the int32 weights are staged
        mf_build_tables(C, in_pad, C.s_a, tid);
    }
    if (tid < kSlots) C.s_ready[tid] = 0;
    if (tid == 0) { C.s_consumed[0] = 0; C.s_consumed[1] = 0; *C.s_abort = 0; P.status[39] = 0; }
#if defined(CCD_PIPE_TRACE)
    for (int i = tid; i < kTraceTasks * 8; i += kPipeThreads) reinterpret_cast<unsigned int*>(ccd_pipe_smem + C.trace_off)[i] = 0u;
#endif

    DecState S;
    S.range = ~uint64_t{0}; S.dist = 0; S.word_pos = 2; S.wbase = 2; S.wbuf = 0; S.n_decoded = 0;
    S.n_part_batches = 0;
    S.prof_wait = 0; S.prof_work = 0; S.stall_ticks = 0; S.stall_events = 0; S.n_rare = 0; S.n_search = 0; S.n_spins = 0;
    for (int i = 0; i < 6; ++i) S.wait_by_j[i] = 0;
    if (wave == 0) {
        // loads through pointers stored in the parameter block are FLAT loads, which the compiler treats as
        // divergent; readfirstlane keeps the coder state (and all control flow depending on it) scalar
        const uint32_t w0 = __builtin_amdgcn_readfirstlane(P.n_words > 0 ? P.words[0] : 0u);
        const uint32_t w1 = __builtin_amdgcn_readfirstlane(P.n_words > 1 ? P.words[1] : 0u);
        S.dist = (static_cast<uint64_t>(w0) << 32) | w1;
        S.wbuf = (S.wbase + lane < P.n_words) ? P.words[S.wbase + lane] : 0u;
    }
    unsigned long long prof[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // [4..7]: MLP sub-phases, [8]: tasks
    const unsigned long long prof_total0 = PROF_T();
    C.seq_base = 0;
    C.px_base = 0;
    __syncthreads();

    unsigned long long prof_ifce = 0, prof_bar = 0;
    for (int g = P.n_grids - 1; g >= 0; --g) {
        const unsigned long long t_if = PROF_T();
        C.H = P.grid_h[g]; C.W = P.grid_w[g];
        C.lat = P.latent[g];
        C.fin = P.ifce_in[g];
        C.fh = (g == P.n_grids - 1) ? C.H : P.grid_h[g + 1];
        C.fw = (g == P.n_grids - 1) ? C.W : P.grid_w[g + 1];
        {   // widest wavefront step of the grid decides the task shape
            const int n_max = wf_longest_step(C.H, C.W);
            // wide steps: 8-pixel tasks (throughput); short steps: the fewer pixels a task holds, the sooner its batch is ready
            C.task_pix = n_max >= CCD_T8 ? 8 : (n_max >= CCD_T4 ? 4 : 2);  // at most ~7 tasks per step: one round of the producers
        }
        // ---- IFCE features at the previously decoded grid's size (coolchic.py:94-146) -------------
        // Per-channel source descriptors and the (tiny) linear layer are staged in LDS first: read through the
        // parameter block inside the loops they would cost a dependent HBM round trip per multiply.
        if (C.fin > 0) {
            const int fin = C.fin, fh = C.fh, fw = C.fw;
            int64_t* s_fw = reinterpret_cast<int64_t*>(static_cast<uint2*>(C.s_tab));                 // [fin][n_if] then bias [n_if] (tables are idle here)
            const int8_t** s_src = reinterpret_cast<const int8_t**>(s_fw + fin * n_if + n_if);  // [fin]
            int32_t* s_gw = reinterpret_cast<int32_t*>(s_src + fin);            // [fin]
            int32_t* s_sh = s_gw + fin;                                          // [fin]
            {
                const int64_t* src = P.ifce + P.ifce_off[g];
                for (int i = tid; i < fin * n_if + n_if; i += kPipeThreads) s_fw[i] = src[i];
                const int base_level = (g == P.n_grids - 1) ? 0 : P.level[g + 1];
                for (int c = tid; c < fin; c += kPipeThreads) {
                    const int m = (g == P.n_grids - 1) ? g : g + 1 + c;
                    s_src[c] = P.latent[m];
                    s_gw[c] = P.grid_w[m];
                    s_sh[c] = (g == P.n_grids - 1) ? 0 : P.level[m] - base_level;
                }
            }
            __syncthreads();
            const bool zero_input = g == P.n_grids - 1;  // first grid: the stack is one all-zero channel (coolchic.py:95-96)
            int16_t* feat = reinterpret_cast<int16_t*>(P.ifce_feat);  // int16 planes; larger features: sentinel + side plane
            const int64_t feat_lim = int64_t{1} << P.feat_bits;
            const int feat_hi_shift = P.feat_bits - 8;  // feat_bits in 8..15
            if (fin <= kIfceFastIn && n_if <= 8 && P.ifce_w32) {
                // The usual shape (<= 12 coarser grids incl. hyperlatents, <= 8 features).  The generic loop below waits for one
                // L2 round trip per input channel and position (~10 k ticks per position, measured); here a position's `fin`
                // bytes are requested together, one position ahead, through explicit global pointers (a FLAT access can only be
                // waited for with vmcnt(0), i.e. together with the previous position's stores).  The weights fit int32
                // (EntropyParams::ifce_w32) and |input << 16| < 2^23: one v_mad_i64_i32 per product gives the reference's wrapping
                // int64 sums exactly; the .to(torch.float) / back round trip around F.interpolate (coolchic.py:142-144) is the
                // identity for the int16 plane and applied by the reader of the side plane (exact_pixel).
                // The loop body is straight-line code on purpose: with branches in it the compiler falls back to
                // s_waitcnt vmcnt(0) everywhere.  Channels >= fin read channel fin - 1 again and meet zero weights; features
                // >= n_if are computed and not stored (the store's predicate is a lane mask).
                // [kIfceFastIn][8] int32 copies of the weights (16-byte rows), zero rows past fin; 16 KB into the idle table region
                // (a pointer rounded up through uintptr_t would lose its LDS address space and turn the reads into FLAT loads)
                int32_t* const s_w32 = reinterpret_cast<int32_t*>(static_cast<uint2*>(C.s_tab) + 2048);
                for (int i = tid; i < kIfceFastIn * 8; i += kPipeThreads) {
                    const int c = i >> 3, j = i & 7;
                    s_w32[i] = (c < fin && j < n_if) ? static_cast<int32_t>(s_fw[c * n_if + j]) : 0;
                }
                __syncthreads();
                // one body for two channel counts: the finest grids of a 7-grid picture stack <= 6 coarser grids - half the loads and
                // multiply-adds of the 12-channel form.  (The pass is bound by the latency of its loads, one position ahead; two or three
                // positions in flight were tried in r04 and ran 4-7 x slower - the compiler then waits with vmcnt(0) between them.)
                const auto pass = [&](auto kin_c) {
                    constexpr int KIN = decltype(kin_c)::value;
                    const glb_ptr<int16_t> featg = (glb_ptr<int16_t>)feat;
                    const glb_ptr<int32_t> wideg = (glb_ptr<int32_t>)P.ifce_wide;
                    const int plane = fh * fw;
                    const int fstride_g = C.fstride;
                    // source descriptors: wave-uniform, read from LDS once (inside the loop each costs an LDS round trip per position)
                    glb_ptr<const int8_t> srcp[KIN];
                    int gwr[KIN], shr[KIN];
#pragma unroll
                    for (int c = 0; c < KIN; ++c) {
                        const int cc = min(c, fin - 1);
                        srcp[c] = (glb_ptr<const int8_t>)reinterpret_cast<const int8_t*>(uni(reinterpret_cast<uint64_t>(s_src[cc])));
                        gwr[c] = uni(s_gw[cc]);
                        shr[c] = uni(s_sh[cc]);
                    }
                    auto fetch = [&](int p, int32_t (&v)[KIN]) {
                        const int y = p / fw, x = p - y * fw;
#pragma unroll
                        for (int c = 0; c < KIN; ++c) v[c] = static_cast<int32_t>(srcp[c][(y >> shr[c]) * gwr[c] + (x >> shr[c])]);
                    };
                    int64_t br[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) br[j] = j < n_if ? s_fw[fin * n_if + j] : 0;
                    int n_if_lane = n_if;
                    asm volatile("" : "+v"(n_if_lane));  // opaque: the stores below are predicated per lane, not branched around
                    const int in_scale = zero_input ? 0 : 65536;  // first grid: the stack is one all-zero channel; else armint.py:193's << 16
                    int32_t v_next[KIN];
                    fetch(min(tid, plane - 1), v_next);
                    for (int p = tid; p < plane; p += kPipeThreads) {
                        int32_t v[KIN];
#pragma unroll
                        for (int c = 0; c < KIN; ++c) v[c] = v_next[c] * in_scale;
                        fetch(min(p + kPipeThreads, plane - 1), v_next);
                        int64_t acc[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[j] = br[j];
#pragma unroll
                        for (int c = 0; c < KIN; ++c) {
                            const int4 w0 = *reinterpret_cast<const int4*>(s_w32 + c * 8), w1 = *reinterpret_cast<const int4*>(s_w32 + c * 8 + 4);
                            // (plain C++, not mad64: an inline-asm statement makes the compiler wait for every outstanding load)
                            const int64_t x = v[c];
                            acc[0] += x * w0.x; acc[1] += x * w0.y; acc[2] += x * w0.z; acc[3] += x * w0.w;
                            acc[4] += x * w1.x; acc[5] += x * w1.y; acc[6] += x * w1.z; acc[7] += x * w1.w;
                        }
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            // |feature| >= 2^feat_bits: sentinel in the int16 plane, the value itself in the int32 side plane
                            // (exactness notes above exact_pixel); both stores are predicated per lane, not branched around.
                            // 32-bit tests: q8 = acc >> 24 lies in [-2^b, 2^b) iff the bits of acc from 24 + b up are all equal.
                            const int32_t hi = static_cast<int32_t>(acc[j] >> 32), q32 = static_cast<int32_t>(acc[j] >> 24);
                            const bool big = static_cast<uint32_t>((hi >> feat_hi_shift) + 1) > 1u || (q32 & 0xffff) == 0x8000;
                            if (j < n_if_lane) featg[p * fstride_g + min(j, n_if - 1)] = (DYN && big) ? kFeatSentinel : static_cast<int16_t>(q32);
                            if (DYN && j < n_if_lane && big) wideg[min(j, n_if - 1) * plane + p] = q32;
                        }
                    }
                };
                if (fin <= 6) pass(std::integral_constant<int, 6>{});
                else pass(std::integral_constant<int, kIfceFastIn>{});
            } else
            for (int p = tid; p < fh * fw; p += kPipeThreads) {
                const int y = p / fw, x = p - y * fw;
                for (int o0 = 0; o0 < n_if; o0 += 8) {
                    uint64_t acc[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = o0 + j < n_if ? static_cast<uint64_t>(s_fw[fin * n_if + o0 + j]) : 0;
                    if (!zero_input) {
                        for (int c = 0; c < fin; ++c) {
                            const int sh = s_sh[c];
                            const uint64_t v = static_cast<uint64_t>(static_cast<int64_t>(s_src[c][(y >> sh) * s_gw[c] + (x >> sh)]) << 16);
#pragma unroll
                            for (int j = 0; j < 8; ++j)
                                if (o0 + j < n_if) acc[j] += v * static_cast<uint64_t>(s_fw[c * n_if + o0 + j]);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (o0 + j < n_if) {
                            const int64_t q8 = static_cast<int64_t>(acc[j]) >> 24;
                            const bool big = static_cast<uint64_t>(q8 + feat_lim - 1) >= static_cast<uint64_t>(2 * feat_lim - 1);
                            feat[p * C.fstride + (o0 + j)] = (DYN && big) ? kFeatSentinel : static_cast<int16_t>(q8);
                            if (DYN && big) P.ifce_wide[(o0 + j) * fh * fw + p] = static_cast<int32_t>(q8);
                        }
                    }
                }
            }
        }
        __syncthreads();  // features visible; every wave finished the previous grid
        PROF_ADD(prof_ifce, t_if);
#if defined(CCD_PIPE_PROFILE) && CCD_PIPE_PROFILE >= 3
        const unsigned long long ifce_grid_ticks = __builtin_amdgcn_s_memtime() - t_if;  // this grid's feature pass (all waves)
#else
        const unsigned long long ifce_grid_ticks = 0;
        (void)ifce_grid_ticks;
#endif

        uint32_t seq_end;
        if (wave == 0) {
            __builtin_amdgcn_s_setprio(3);
#ifdef CCD_PIPE_PROFILE
            const unsigned long long k0 = S.prof_work;
            const unsigned long long g_t0 = __builtin_amdgcn_s_memtime(), sp0 = S.n_spins, se0 = S.stall_events;
#endif
            seq_end = decoder_grid<MF>(C, S);
            __builtin_amdgcn_s_setprio(0);
#ifdef CCD_PIPE_PROFILE
            if (lane == 0 && g == 0)
                for (int i = 0; i < 6; ++i) P.status[32 + i] = static_cast<int32_t>(S.wait_by_j[i] >> 10);
            if (lane == 0 && g < 4) {  // per-grid decoder counters for the four finest grids: status[24 + 2 g ..]
                P.status[24 + 2 * g] = static_cast<int32_t>(ifce_grid_ticks >> 10);  // level 3: ticks of the IFCE feature pass before this grid
                P.status[25 + 2 * g] = static_cast<int32_t>((S.prof_work - k0) >> 10);
                // light counters: total ticks of the grid, ticks stalled on producers, number of stalls
                P.status[50 + 3 * g] = static_cast<int32_t>((__builtin_amdgcn_s_memtime() - g_t0) >> 10);
                P.status[51 + 3 * g] = static_cast<int32_t>(S.n_spins - sp0);  // polls of a ready counter inside the asm region
                P.status[52 + 3 * g] = static_cast<int32_t>(S.stall_events - se0);
            }
#endif
        } else {
            // the matrix-core evaluation only serves the 8-pixel tasks of wide grids: its chain has the same length whatever
            // the number of pixels, while the vector-ALU code of a 4- / 2-pixel task spreads a pixel over 16 / 32 lanes
            GridSeg segs[3];
            const int n_segs = grid_segments(static_cast<uint32_t>(C.H), static_cast<uint32_t>(C.W), C.task_pix, segs);
            const uint32_t grid_seq_base = C.seq_base;
            seq_end = grid_seq_base;
            for (int si = 0; si < n_segs; ++si) {
                const int tp = segs[si].task_pix;
                C.seq_base = seq_end;  // (batches are numbered through the segments)
                seq_end = tp == 8 ? producer_grid<NV, 8, MF, MF, DYN, SH>(C, prof, segs[si])
                                  : (tp == 4 ? producer_grid<NV, 16, false, MF, DYN, SH>(C, prof, segs[si]) : producer_grid<NV, 32, false, MF, DYN, SH>(C, prof, segs[si]));
                if (lds_load_acquire(C.s_abort) != 0) break;
            }
            C.seq_base = grid_seq_base;
        }
        const unsigned long long t_b = PROF_T();
        __syncthreads();  // also makes the decoder's global writes of this grid visible to every wave
        PROF_ADD(prof_bar, t_b);
        if (lds_load_acquire(C.s_abort) != 0) break;
        C.seq_base = seq_end;  // every wave walked the same batches
        C.px_base += static_cast<uint32_t>(C.H) * static_cast<uint32_t>(C.W);
    }
#if defined(CCD_PIPE_TRACE)
    {
                const unsigned int* t = reinterpret_cast<const unsigned int*>(ccd_pipe_smem + C.trace_off);
        for (int i = tid; i < kTraceTasks * 8; i += kPipeThreads) g_trace[i] = t[i];
    }
#endif
    if (tid == 0) {
        const uint32_t ab = *C.s_abort;
        P.status[0] = ab ? -static_cast<int32_t>(ab) : 0;
        P.status[1] = static_cast<int32_t>(S.word_pos);
#ifndef CCD_PIPE_PROFILE
        P.status[37] = static_cast<int32_t>(S.n_part_batches);  // batches the decoder took part by part (tests)
        {   // grids whose body ran as one stream of pixels (StreamBody; tests)
            int n_streamed = 0;
            for (int g2 = 0; g2 < P.n_grids; ++g2) {
                const int gh = P.grid_h[g2], gw = P.grid_w[g2];
                const int n_max = wf_longest_step(gh, gw);
                StreamBody sb;
                sb.init(static_cast<uint32_t>(gh), static_cast<uint32_t>(gw), n_max >= CCD_T8 ? 8 : (n_max >= CCD_T4 ? 4 : 2));
                n_streamed += sb.on ? 1 : 0;
            }
            P.status[36] = n_streamed;
        }
#endif
        // symbols that left the asm region's common path (renormalisations that need a payload refill aside): window misses
        // and sentinels [62], of which full 128-way searches [63] - what a stream's statistics cost the decoder (bench.py)
        P.status[62] = static_cast<int32_t>(S.n_rare); P.status[63] = static_cast<int32_t>(S.n_search);
        {   // symbols decoded = all grids unless aborted
            uint64_t n_sym = 0;
            for (int g2 = 0; g2 < P.n_grids; ++g2) n_sym += static_cast<uint64_t>(P.grid_h[g2]) * P.grid_w[g2];
            if (ab) n_sym = 0;
            P.status[2] = static_cast<int32_t>(n_sym & 0xffffffffu);
            P.status[3] = static_cast<int32_t>(n_sym >> 32);
        }
    }
#ifdef CCD_PIPE_PROFILE
    if (lane == 0 && wave < 2) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(P.status + 4) + wave * 5;
        o[0] = __builtin_amdgcn_s_memtime() - prof_total0;
        if (wave == 0) {
            o[1] = S.prof_wait; o[2] = S.prof_work; o[3] = prof_ifce; o[4] = prof_bar;
            P.status[38] = static_cast<int32_t>(S.n_spins);  // polls of ready counters inside the decoder's asm region (~250 ticks each)  // leaves of the asm loop, full searches
        }
        else {
            o[1] = prof[0]; o[2] = prof[1]; o[3] = prof[2]; o[4] = prof[3];
            unsigned long long* e = reinterpret_cast<unsigned long long*>(P.status + 40);
            for (int i = 0; i < 5; ++i) e[i] = prof[4 + i];
        }
    }
#else
    (void)prof_total0; (void)prof_ifce; (void)prof_bar;
#endif
}

size_t entropy_pipe_lds_bytes(int dim, int n_layers, int ring_rows, int mfma) {
    size_t n = pipe_layout(dim, n_layers, (dim + 3) & ~3, ring_rows, mfma ? mf_tables(n_layers) : 0).end;
#if defined(CCD_PIPE_TRACE)
    n += kTraceLdsBytes;
#endif
    return n;
}

// rows of the decoded-symbol ring for a stream whose widest grid is max_grid_w (0: too wide for the kernel)
int entropy_pipe_ring_rows(int max_grid_w) {
    const int need = ring_rows_needed(max_grid_w);
    if (need > kRingRows) return 0;
    int r = 64;
    while (r < need) r *= 2;
    return r;
}

// `operands_ok`: the static part of the 32-bit operand envelope (FixedArm::w32 && Network::feat_i32, ccd_format.cpp); the
// data-dependent part is checked on the device (exact_pixel).  The vector-ALU kernel always carries the full ring.
bool entropy_pipe_supports(int dim, int n_layers, int operands_ok, int max_grid_w) {
    const int ring = entropy_pipe_ring_rows(max_grid_w);
    return operands_ok && dim <= 4 * kMaxNV && n_layers <= 8 && ring > 0 && entropy_pipe_lds_bytes(dim, n_layers, kRingRows, 0) <= 160 * 1024;
}

// The matrix-core evaluation of the ARM (see the MF notes above producer_grid); max_abs_weight over every ARM layer
// and the stabiliser, max_feature_bound = the worst case of an IFCE feature (ccd::worst_feature_bound: a feature lies in
// [-bound, bound - 1]).  The limits are those of the signed digits, not of the bit width: three digits hold
// -0x808080 .. 0x7F7F7F and two hold -0x8080 .. 0x7F7F = 32 639 (tests/test_arm_envelope.py sits on both).
bool entropy_pipe_supports_mfma(int dim, int n_layers, int n_ifce_out, int narrow, int max_grid_w, long long max_abs_weight,
                                long long max_feature_bound) {
    const int ring = entropy_pipe_ring_rows(max_grid_w);
    return narrow && ring > 0 && dim <= 20 && n_layers >= 2 && n_layers <= 8 && n_ifce_out <= 8 &&
           max_abs_weight <= kMfMaxDigits3 && max_feature_bound <= kMfMaxDigits2 + 1 &&
           entropy_pipe_lds_bytes(dim, n_layers, ring, 1) <= 160 * 1024;
}

// ---- debug: every left cumulative the producers can compute for a run of scale indices -------------------------------
// out[(c - scale_first) * 32768 * 127 + mu_idx * 127 + (s + 63)] = window_left_d256(256 (x - mu), rcp / 256, s) for s = -63 .. 63 (s = -64 is 0
// and the right bound of s is the left bound of s + 1): 32768 x 2561 x 127 = 1.0658e10 values in all (tools/cdf_sweep.py).
__global__ void laplace_sweep_pipe_kernel(const float* scale_table, const double* rcp_table, int scale_first, int n_scales, uint32_t* out) {
    const int64_t n = static_cast<int64_t>(n_scales) * kNumMu * 127;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int s = static_cast<int>(i % 127) - 63;
        const int64_t r = i / 127;
        const int mu_idx = static_cast<int>(r % kNumMu), c = scale_first + static_cast<int>(r / kNumMu);
        out[i] = window_left_d256(window_d256(mu_idx, s), window_rcp256(rcp_table[c]), s, kExpTab);  // what the producers run
    }
}
hipError_t launch_laplace_sweep_pipe(const float* scale_table, const double* rcp_table, int scale_first, int n_scales, uint32_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(laplace_sweep_pipe_kernel, dim3(256 * 16), dim3(256), 0, stream, scale_table, rcp_table, scale_first, n_scales, out);
    return hipGetLastError();
}

template <int NV, bool MF, bool DYN, class SH = ShapeDyn>
static hipError_t launch_pipe_nv(const EntropyParams* d_slots, int n_slots, size_t lds_bytes, hipStream_t stream) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(entropy_pipe_kernel<NV, MF, DYN, SH>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((entropy_pipe_kernel<NV, MF, DYN, SH>), dim3(n_slots), dim3(kPipeThreads), lds_bytes, stream, d_slots);
    return hipGetLastError();
}

// the shapes with a compile-time instantiation (launch_entropy_pipe's `shape`): 0 = none, 1 = ShapeHop
int entropy_pipe_fixed_shape(int dim, int n_layers, int n_spatial) {
    return (dim == ShapeHop::dim && n_layers == ShapeHop::n_layers && n_spatial == ShapeHop::n_sp) ? 1 : 0;
}

// One kernel per width nv: the matrix-core variant serves nv = 1 .. 5 (dim <= 20), the others 1 .. 8.
template <bool MF, bool DYN>
static hipError_t launch_pipe(int nv, const EntropyParams* d_slots, int n_slots, size_t lds_bytes, hipStream_t stream) {
    if (MF && nv > 5) return hipErrorInvalidValue;
    switch (nv) {
        case 1: return launch_pipe_nv<1, MF, DYN>(d_slots, n_slots, lds_bytes, stream);
        case 2: return launch_pipe_nv<2, MF, DYN>(d_slots, n_slots, lds_bytes, stream);
        case 3: return launch_pipe_nv<3, MF, DYN>(d_slots, n_slots, lds_bytes, stream);
        case 4: return launch_pipe_nv<4, MF, DYN>(d_slots, n_slots, lds_bytes, stream);
        case 5: return launch_pipe_nv<5, MF, DYN>(d_slots, n_slots, lds_bytes, stream);
        case 6: return launch_pipe_nv<MF ? 5 : 6, MF, DYN>(d_slots, n_slots, lds_bytes, stream);  // (MF: not reached, and no sixth kernel)
        case 7: return launch_pipe_nv<MF ? 5 : 7, MF, DYN>(d_slots, n_slots, lds_bytes, stream);
        case 8: return launch_pipe_nv<MF ? 5 : 8, MF, DYN>(d_slots, n_slots, lds_bytes, stream);
        default: return hipErrorInvalidValue;
    }
}
// All `n_slots` descriptors must share nv = ceil(dim / 4), the mfma flag, the dyn flag and the fixed shape (the host groups the
// slots of a batch by all four).  The matrix-core variant's envelope implies dyn = 0 and shape = 0.
hipError_t launch_entropy_pipe(const EntropyParams* d_slots, int n_slots, int nv, int mfma, int dyn, int shape, size_t lds_bytes, hipStream_t stream) {
    if (n_slots <= 0) return hipSuccess;
    if (shape == 1 && !mfma && nv == 5)
        return dyn ? launch_pipe_nv<5, false, true, ShapeHop>(d_slots, n_slots, lds_bytes, stream)
                   : launch_pipe_nv<5, false, false, ShapeHop>(d_slots, n_slots, lds_bytes, stream);
    if (shape != 0) return hipErrorInvalidValue;
    if (mfma) return launch_pipe<true, false>(nv, d_slots, n_slots, lds_bytes, stream);
    return dyn ? launch_pipe<false, true>(nv, d_slots, n_slots, lds_bytes, stream) : launch_pipe<false, false>(nv, d_slots, n_slots, lds_bytes, stream);
}

}  // namespace ccd

// Host only (tests): the walks of ccd_wavefront.hpp as this translation unit compiles them (include/ccd.h).
extern "C" int64_t ccd_debug_grid_walk(int h, int w, int task_pix, int which, int32_t* steps, int64_t cap, int32_t* segs, int32_t* n_segs) {
    using namespace ccd;
    if (h < 1 || w < 1 || h > kWfMaxSide || w > kWfMaxSide || (task_pix != 2 && task_pix != 4 && task_pix != 8) || which < 0 || which > 4 ||
        cap < 0 || (segs && !n_segs))
        return CCD_ERR_ARG;
    if (segs) {
        GridSeg gs[3];
        *n_segs = grid_segments(static_cast<uint32_t>(h), static_cast<uint32_t>(w), task_pix, gs);
        for (int i = 0; i < *n_segs; ++i) {
            const int32_t row[6] = {static_cast<int32_t>(gs[i].first), static_cast<int32_t>(gs[i].steps), static_cast<int32_t>(gs[i].pix_before),
                                    static_cast<int32_t>(gs[i].n_pix), gs[i].task_pix, gs[i].body ? 1 : 0};
            for (int k = 0; k < 6; ++k) segs[i * 6 + k] = row[k];
        }
    }
    int64_t c = 0;
    const auto put = [&](uint32_t y0, uint32_t x0, uint32_t n, uint32_t moved, uint32_t left) {
        if (steps && c < cap) {
            const uint32_t row[5] = {y0, x0, n, moved, left};
            for (int k = 0; k < 5; ++k) steps[c * 5 + k] = static_cast<int32_t>(row[k]);
        }
        ++c;
    };
    if (which == 1) {
        StepIter it;
        it.init(h, w);
        while (it.next()) put(it.y0, it.x0, it.n, 0u, 0u);
    } else if (which == 3) {
        const int n_steps = wf_n_steps(h, w);
        for (int s = 0; s < n_steps; ++s) {
            int y0, x0;
            const int n = wf_step(h, w, s, y0, x0);
            put(y0, x0, n, wf_moved(w, s) ? 1u : 0u, static_cast<uint32_t>(n_steps - 1 - s));
        }
    } else {
        StepWalk it;
        it.init(static_cast<uint32_t>(h), static_cast<uint32_t>(w));
        while (it.next()) {
            if (which == 4 && !it.raster) it.seek_before(static_cast<uint32_t>(c) + 1u);  // this step's state again, all from the closed forms
            put(it.y0, it.x0, it.n, it.moved, it.left);
            if (which == 2 && !it.raster && it.left > 0) it.seek_before(static_cast<uint32_t>(c));  // a fresh state for step c
        }
    }
    return c;
}
extern "C" int ccd_debug_stream_min_step(void) { return static_cast<int>(ccd::kStreamMinStep); }

#if defined(CCD_PIPE_TRACE)
// trace builds only (tools/trace_tasks.py): which grid / first task to record, and the records back
extern "C" int ccd_debug_trace_config(unsigned int grid_w, unsigned int steps_left) {
    const unsigned int cfg[2] = {grid_w, steps_left};
    return hipMemcpyToSymbol(HIP_SYMBOL(ccd::g_trace_cfg), cfg, sizeof(cfg)) == hipSuccess ? 0 : -1;
}
extern "C" int ccd_debug_trace_read(unsigned int* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ccd::g_trace), sizeof(unsigned int) * ccd::kTraceTasks * 8) == hipSuccess ? 0 : -1;
}
#endif
