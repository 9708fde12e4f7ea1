// ccd_wavefront.hpp - the ORDER in which the latents of a grid are coded (latent.py:66-140), stated once for both writers, both
// entropy kernels and the batch planner: raster, one pixel per step, for a grid at most 9 wide; otherwise steps c = x + 10 y, the
// pixels of a step in increasing y.  The literals 10 and 9 (and 0xcccd, a division by ten) stand in this header only; all of it
// is __host__ __device__, and ccd_debug_grid_walk (ccd_entropy_pipe.hip) runs it on the host for tests/test_stream_body_math.py.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ccd {

constexpr int kWfSlope = 10;      // x + kWfSlope y is constant along a step: pixel i of a step is (y0 + i, x0 - kWfSlope i)
constexpr int kWfMaxSide = 16383; // the header's 14-bit picture sizes (header.py:244-307): no grid is higher or wider

// (the device library's min is not declared in a plain C++ translation unit)
template <typename T>
__host__ __device__ constexpr T wf_min(T a, T b) { return a < b ? a : b; }

// (int or uint32_t: the kernels keep some of their walks unsigned)
template <typename T>
__host__ __device__ constexpr bool wf_raster(T W) { return W <= T(9); }
template <typename T>
__host__ __device__ constexpr T wf_n_steps(T H, T W) { return wf_raster(W) ? H * W : W + T(10) * (H - T(1)); }
// the step that holds (y, x) of a wavefront grid, and a step's first row
__host__ __device__ constexpr int wf_step_of(int y, int x) { return x + 10 * y; }
__host__ __device__ constexpr int wf_first_row(int W, int c) { return c < W ? 0 : (c - W) / 10 + 1; }
// step c of an H x W grid: its first pixel; returns its length
__host__ __device__ inline int wf_step(int H, int W, int c, int& y0, int& x0) {
    if (wf_raster(W)) { y0 = c / W; x0 = c - y0 * W; return 1; }
    if (c < W) { y0 = 0; x0 = c; }
    else { y0 = (c - W) / 10 + 1; x0 = W - 10 + (c - W) % 10; }
    return wf_min(H - y0, x0 / 10 + 1);
}
// whether step c begins a row below step c - 1
__host__ __device__ constexpr bool wf_moved(int W, int c) { return c >= W && (c - W) % (wf_raster(W) ? W : 10) == 0; }
__host__ __device__ constexpr int wf_longest_step(int H, int W) { return wf_raster(W) ? 1 : wf_min(H, (W - 1) / 10 + 1); }

// The pipelined kernel's ring of decoded symbols: 64 cells per row, a pixel's column in it is its step (mod 64), so the cells of
// a step's pixels - and of one pixel's context - never collide while ring_rows_needed(W) rows are kept.
__host__ __device__ constexpr int ring_cell(int y, int x, int ring_mask) { return (y & ring_mask) * 64 + ((x + 10 * y) & 63); }
__host__ __device__ constexpr int ring_rows_needed(int W) { return W / 10 + 6; }

// x / 10 without a division, for the walks on the path between two tasks: exact below 43699, so for every column of a grid
__host__ __device__ constexpr uint32_t wf_div10(uint32_t x) { return (x * 0xcccdu) >> 19; }
static_assert(kWfMaxSide < 43699, "StepWalk::next: the multiply-shift must be exact for every column of the widest grid");

// The producers' walk over the steps of a grid (same order as StepIter below), kept incremental and unsigned: a producer
// passes every step on the way to its next task, so this is on the path between two tasks.
struct StepWalk {
    uint32_t H, W, raster, left;
    uint32_t y0, x0, n, moved;  // moved: the step's first row is one below the previous step's
    __host__ __device__ void init(uint32_t h, uint32_t w) {
        H = h; W = w; raster = w <= 9u; left = raster ? h * w : w + 10u * (h - 1u);
        y0 = 0; x0 = ~0u; n = 0; moved = 0;
    }
    __host__ __device__ bool next() {
        if (left == 0) return false;
        --left;
        ++x0;
        moved = x0 == W;
        if (moved) { x0 = raster ? 0u : W - 10u; ++y0; }
        n = raster ? 1u : wf_min(H - y0, wf_div10(x0) + 1u);  // x0 / 10 + 1, as (x0 * 0xcccd) >> 19
        return true;
    }
    // length of step c / whether its start lies a row below step c - 1's (wavefront order)
    __host__ __device__ uint32_t len_of(uint32_t c) const {
        const uint32_t yy = c < W ? 0u : (c - W) / 10u + 1u, xx = c < W ? c : W - 10u + (c - W) % 10u;
        return wf_min(H - yy, xx / 10u + 1u);
    }
    __host__ __device__ uint32_t moved_at(uint32_t c) const { return (c >= W && (c - W) % 10u == 0u) ? 1u : 0u; }
    // the state of step c - 1 (c >= 1, wavefront order): next() then arrives at step c
    __host__ __device__ void seek_before(uint32_t c) {
        const uint32_t p = c - 1u;
        y0 = p < W ? 0u : (p - W) / 10u + 1u;
        x0 = p < W ? p : W - 10u + (p - W) % 10u;
        n = len_of(p); moved = moved_at(p);
        left = W + 10u * (H - 1u) - c;
    }
};

// Iterates the wavefront steps of one grid (latent.py:66-140).
struct StepIter {
    int H, W, raster, n_steps;
    int c, y0, x0, n;
    __host__ __device__ void init(int h, int w) { H = h; W = w; raster = w <= 9; n_steps = raster ? h * w : w + 10 * (h - 1); c = -1; }
    __host__ __device__ bool seek(int step) { c = step - 1; return next(); }
    __host__ __device__ bool next() {
        if (++c >= n_steps) return false;
        if (raster) { y0 = c / W; x0 = c - y0 * W; n = 1; }
        else {
            if (c < W) { y0 = 0; x0 = c; }
            else { y0 = (c - W) / 10 + 1; x0 = W - 10 + (c - W) % 10; }
            n = wf_min(H - y0, x0 / 10 + 1);
        }
        return true;
    }
};

// ---- The BODY of a wide grid as one stream of pixels (r04).  Steps of the wavefront order are independent of batch boundaries as
// soon as a pixel's left neighbour (same index in the previous step) lies at least a task + a batch behind it in decoding order,
// i.e. for steps of >= 18 pixels.  So the steps [first, end) whose length is >= kStreamMinStep - 1 - all of a grid but the ramps at
// its two corners - are cut into 16-pixel batches / 8-pixel tasks WITHOUT regard to step ends: every batch but the last is full
// (the unrolled block), no 3-pixel tail batch and no step hand-over per step, 6.4 instead of 7 tasks per step of a portrait
// Kodak picture.  A task then holds pixels of up to two steps (per-lane position select), the decoder sees ONE step of n_body
// symbols (it takes each pixel's ring cell and latent offset from the row meta the producers write).
//   ramp-up:  steps c < first = 10 (T - 1): y0 = 0, n = c / 10 + 1 < T, together 5 T (T - 1) pixels;
//   ramp-down: steps c >= end = W + 10 (H - T): fewer than T rows left, again 5 T (T - 1) pixels (the mirror image);
//   in between n = min(H - y0, x0 / 10 + 1) >= T - 1 (x0 >= W - 10 >= 10 (T - 1) - 9 behind the first row).
#ifndef CCD_STREAM_MIN_STEP
#define CCD_STREAM_MIN_STEP 24
#endif
constexpr uint32_t kStreamMinStep = CCD_STREAM_MIN_STEP;
static_assert(kStreamMinStep >= 19, "a streamed task must find its left neighbours in an EARLIER batch: steps of >= 18 pixels");
struct StreamBody {
    uint32_t first, end, n_pix, pix_before;  // steps [first, end), pixels of the body, pixels of the grid in front of it
    bool on;
    __host__ __device__ void init(uint32_t H, uint32_t W, int task_pix) {
        const uint32_t T = kStreamMinStep;
        on = task_pix == 8 && W > 10u * (T - 1u) && H >= T;  // (4-pixel tasks streamed: measured slower, r04 and r06)
        {   // where it pays: long steps (the decoder is the limit: its per-step costs go away) or steps whose last task is mostly empty.
            // Elsewhere - 39-pixel steps = 8 + 8 + 8 + 8 + 7 - the tasks of step-aligned batches wait for ONE earlier task each instead
            // of two (profiles/r04/ab_entropy_stream.txt: grid 1 of a landscape Kodak picture 16.8 -> 17.3 M ticks when streamed).
            const uint32_t n_pl = (W - 1u) / 10u + 1u, tail = n_pl & 7u;
            on = on && (n_pl >= 48u || (tail >= 1u && tail <= 4u));
        }
        first = 10u * (T - 1u);
        end = on ? W + 10u * (H - T) : 0u;
        pix_before = 5u * T * (T - 1u);
        n_pix = on ? H * W - 2u * pix_before : 0u;
    }
};

// Segments of a grid, the same list for the decoder and for every producer: all steps - or, around a streamed body, the ramp in
// front of it, the body (ONE step of n_pix symbols for the decoder), the ramp behind it.  The ramps of a streamed grid - 230 steps
// of 1 .. 23 pixels at each of two corners, every one a full "late work + hand-overs + one part" chain - run 4-pixel tasks
// (shorter late path, 4 symbols instead of 8 between "ready" and "published"); same batches of 16, so nothing drains in between.
#ifndef CCD_RAMP_TASK_PIX
#define CCD_RAMP_TASK_PIX 4
#endif
static_assert(CCD_RAMP_TASK_PIX == 4 || CCD_RAMP_TASK_PIX == 8, "ramps and body share the 16-pixel batches: 2-pixel tasks (8-pixel batches) would need the slots drained between segments");
struct GridSeg { uint32_t first, steps, pix_before, n_pix; int task_pix; bool body; };  // steps [first, first + steps), pixels in front of / in them
__host__ __device__ __forceinline__ int grid_segments(uint32_t H, uint32_t W, int task_pix, GridSeg* out) {
    StreamBody b;
    b.init(H, W, task_pix);
    const uint32_t total = wf_n_steps(H, W);
    if (!b.on) { out[0] = GridSeg{0u, total, 0u, H * W, task_pix, false}; return 1; }
    out[0] = GridSeg{0u, b.first, 0u, b.pix_before, CCD_RAMP_TASK_PIX, false};
    out[1] = GridSeg{b.first, b.end - b.first, b.pix_before, b.n_pix, task_pix, true};
    out[2] = GridSeg{b.end, total - b.end, H * W - b.pix_before, b.pix_before, CCD_RAMP_TASK_PIX, false};
    return 3;
}

}  // namespace ccd
