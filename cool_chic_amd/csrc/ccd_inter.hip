// ccd_inter.hip - P / B frame reconstruction on the device (SURVEY.md section 8f "next-1").
//
// Reference behaviour (paths relative to /root/reference/coolchic):
//   bitstream/decode.py:156-189                      global shift, warp, alpha / beta blend, + residue
//   component/intercoding/globalmotion.py:151-160    integer global translation (nearest, border clamp)
//   component/intercoding/warp.py:226-243,294-397    sinc-windowed N-tap warp, TRAINING mode (the decoder never
//                                                    calls .eval(): flows are NOT quantised), border clamp;
//                                                    2 / 4 taps = F.grid_sample bilinear / bicubic (warp.py:325-343)
//   io/format/yuv.py:303-316                         4:2:0 references -> 4:4:4 by nearest x2
//
// Numerics: identical formulas to oracle/cc_oracle.c section 11 (sin / cos in f64 with explicit fma, rounded to
// f32; separable passes accumulated with fmaf, taps ascending) -> bit-identical to the oracle.
#include <hip/hip_runtime.h>

#include "ccd_device.hpp"
#include "ccd_kernels.hpp"
#include "ccd_planes.hpp"
#include "ccd_trig.hpp"

namespace ccd {

__device__ __forceinline__ int ic_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A 256-thread workgroup owns a 64 x 4 tile of pixels: the thread's pixel in tile (tx, ty), and the grid whose tiles cover h x w.
__device__ __forceinline__ void tile_pixel(unsigned tx, unsigned ty, int* x, int* y) { *x = tx * 64 + (threadIdx.x & 63); *y = ty * 4 + (threadIdx.x >> 6); }
static dim3 tile_grid(int h, int w) { return dim3((w + 63) / 64, (h + 3) / 4); }

__device__ __forceinline__ void ic_sincos(float a, float* s_out, float* c_out) {  // cores and reduction: ccd_trig.hpp
    int n;
    const double r = trig_reduce(static_cast<double>(a), &n);
    const double sn = trig_sin_core(r), cs = trig_cos_core(r);
    double sv = (n & 1) ? cs : sn, cv = (n & 1) ? sn : cs;
    if (n & 2) sv = -sv;
    if (n == 1 || n == 2) cv = -cv;
    *s_out = static_cast<float>(sv);
    *c_out = static_cast<float>(cv);
}

// Integer planes of a decoded frame -> the [3][H][W] float tensor the warper reads (value = q / (2^bd - 1),
// 4:2:0 chroma repeated 2x2).
template <typename T>
__device__ __forceinline__ void planes_to_444_pixel(const T* p0, const T* p1, const T* p2, float* out, int h, int w, int chroma_half, float maxv, int x, int y) {
    const size_t plane = static_cast<size_t>(h) * w, i = static_cast<size_t>(y) * w + x;
    out[i] = static_cast<float>(p0[i]) / maxv;
    const int cw = chroma_half ? w / 2 : w;
    const size_t ci = chroma_half ? static_cast<size_t>(y >> 1) * cw + (x >> 1) : i;
    out[plane + i] = static_cast<float>(p1[ci]) / maxv;
    out[2 * plane + i] = static_cast<float>(p2[ci]) / maxv;
}
template <typename T>
__global__ void planes_to_444_kernel(const T* p0, const T* p1, const T* p2, float* out, int h, int w, int chroma_half, float maxv) {
    int x, y;
    tile_pixel(blockIdx.x, blockIdx.y, &x, &y);
    if (x >= w || y >= h) return;
    planes_to_444_pixel(p0, p1, p2, out, h, w, chroma_half, maxv, x, y);
}
// The same conversion of many frames in one launch (the reference items of a ccd_iscore run): a job is one frame,
// its workgroups - the 64 x 4 pixel tiles of planes_to_444_kernel - find it in a prefix table.  Every output word has one writer.
__global__ __launch_bounds__(256) void planes_to_444_jobs_kernel(const PlanesConvJob* __restrict__ jobs, const uint32_t* __restrict__ prefix, int n_jobs) {
    const int j = entry_of(prefix, n_jobs, blockIdx.x);
    const PlanesConvJob& C = jobs[j];  // (uniform: scalar loads)
    const uint32_t local = blockIdx.x - prefix[j], tiles_x = static_cast<uint32_t>(C.tiles_x);
    int x, y;
    tile_pixel(local % tiles_x, local / tiles_x, &x, &y);
    if (x >= C.w || y >= C.h) return;
    if (C.wide)
        planes_to_444_pixel(static_cast<const uint16_t*>(C.p[0]), static_cast<const uint16_t*>(C.p[1]), static_cast<const uint16_t*>(C.p[2]), C.out, C.h, C.w,
                            C.chroma_half, C.maxv, x, y);
    else
        planes_to_444_pixel(static_cast<const uint8_t*>(C.p[0]), static_cast<const uint8_t*>(C.p[1]), static_cast<const uint8_t*>(C.p[2]), C.out, C.h, C.w,
                            C.chroma_half, C.maxv, x, y);
}
hipError_t launch_planes_to_444_jobs(const PlanesConvJob* d_jobs, const uint32_t* d_prefix, int n_jobs, uint32_t n_blocks, hipStream_t stream) {
    if (n_jobs <= 0 || n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(planes_to_444_jobs_kernel, dim3(n_blocks), dim3(256), 0, stream, d_jobs, d_prefix, n_jobs);
    return hipGetLastError();
}

hipError_t launch_planes_to_444(const void* p0, const void* p1, const void* p2, float* out, int h, int w, int bitdepth,
                                int frame_data_type, hipStream_t stream) {
    const dim3 grid = tile_grid(h, w);
    const float maxv = static_cast<float>((1 << bitdepth) - 1);
    const int half = frame_data_type == 1;
    if (bitdepth == 8)
        hipLaunchKernelGGL(planes_to_444_kernel<uint8_t>, grid, dim3(256), 0, stream, static_cast<const uint8_t*>(p0),
                           static_cast<const uint8_t*>(p1), static_cast<const uint8_t*>(p2), out, h, w, half, maxv);
    else
        hipLaunchKernelGGL(planes_to_444_kernel<uint16_t>, grid, dim3(256), 0, stream, static_cast<const uint16_t*>(p0),
                           static_cast<const uint16_t*>(p1), static_cast<const uint16_t*>(p2), out, h, w, half, maxv);
    return hipGetLastError();
}

// the integer part of a flow as a tap offset, saturated to +-(size + 16) (oracle/cc_oracle.c tap_offset): taps beyond lie past the
// border on the same side, so in-range flows keep their taps and far ones (|flow| >= 2^31 included) read the border; NaN -> lower bound
__device__ __forceinline__ int ic_tap_offset(float f, int size) {
    return static_cast<int>(fminf(fmaxf(f, -static_cast<float>(size + 16)), static_cast<float>(size + 16)));
}
// ---- WHERE a window reads, stated once for the warps and for dsens_dep_kernel (ic_window_axis).  Along an axis of n samples a
// window is nt taps at consecutive integer positions from a first one; the tap at position t reads the reference at ic_tap_index:
// border clamp, integer global shift, border clamp - monotone in t, so a window reads inside [index(first), index(first + nt - 1)].
__device__ __forceinline__ int ic_tap_index(int t, int n, int g) { return ic_clamp(ic_clamp(t, 0, n - 1) + g, 0, n - 1); }
// position of tap j of the sinc window around sample i with the tap offset r of its flow
__device__ __forceinline__ int ic_sinc_tap(int i, int nt, int j, int r) { return i + (-(nt / 2) + 1) + j + r; }

// ---- the sinc-windowed warp, templated on the tap count.  NT > 0: known at compile time, arrays of NT, every loop fully unrolled;
// NT == 0: n_taps at run time, arrays of kMaxTaps, loops rolled.  r06: the run-time version keeps cx / cy / xs in scratch memory
// (dynamic indexing of per-thread arrays) and spent 0.5 ms per 1080p frame there - ccd_decode_video's 31 inter frames were 21 ms of a
// 190 ms call (profiles/r06/gop_timing_before.txt) - so the sinc-8 warp of every preset has its own instantiation.  Same operations
// in the same order: bit-identical.
// (r06, measured and dropped: evaluating only the polynomial the quadrant needs where a wave agrees on it - the window's cos does,
// per tap - behind a ballot: bit-exact, and 0.55 ms per 1080p frame instead of 0.34: the scalar branches serialise what the
// scheduler interleaves when all 32 evaluations of a pixel are straight-line code.)
constexpr int kMaxTaps = 16;
template <int NT> constexpr int kTapCap = NT > 0 ? NT : kMaxTaps;  // size of an array over the taps
template <int NT> constexpr int kTapUnroll = NT > 0 ? NT : 1;       // unroll count of a loop over them (a bare `unroll` half-unrolls NT == 0)

// warp.py:238-243
template <int NT>
__device__ __forceinline__ void ic_coeffs(float s, int n_taps, float (&coef)[kTapCap<NT>]) {
    constexpr int kUnroll = kTapUnroll<NT>;
    const int nt = NT > 0 ? NT : n_taps;
    const float pi_f = 3.14159265358979323846f;
#pragma unroll kUnroll
    for (int j = 0; j < nt; ++j) {
        const float d = s - static_cast<float>(j - nt / 2 + 1);
        float sn, unused_c, unused_s, win;
        ic_sincos(pi_f * d / static_cast<float>(nt), &unused_s, &win);
        float snc = 1.0f;
        if (d != 0.0f) { const float a = pi_f * d; ic_sincos(a, &sn, &unused_c); snc = sn / a; }
        coef[j] = win * snc;
    }
}
// the N x N taps of one pixel from its coefficients (rows accumulate in ascending order per channel: the oracle's chain)
template <int NT>
__device__ __forceinline__ void ic_taps(const float* __restrict__ ref, int H, int W, int gx, int gy, int n_taps, int rx, int ry,
                                        const float (&cx)[kTapCap<NT>], const float (&cy)[kTapCap<NT>], int y, int x, float out[3]) {
    constexpr int kUnroll = kTapUnroll<NT>;
    const int nt = NT > 0 ? NT : n_taps;
    const size_t plane = static_cast<size_t>(H) * W;
    int xs[kTapCap<NT>];
#pragma unroll kUnroll
    for (int j = 0; j < nt; ++j) xs[j] = ic_tap_index(ic_sinc_tap(x, nt, j, rx), W, gx);
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll kUnroll
    for (int i = 0; i < nt; ++i) {
        const int yy = ic_tap_index(ic_sinc_tap(y, nt, i, ry), H, gy);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* row = ref + c * plane + static_cast<size_t>(yy) * W;
            float line = 0.0f;
#pragma unroll kUnroll
            for (int j = 0; j < nt; ++j) line = __fmaf_rn(row[xs[j]], cx[j], line);
            acc[c] = __fmaf_rn(line, cy[i], acc[c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = acc[c];
}

// ---- warp_filter_size 2 / 4: the Warper's native path = F.grid_sample(bilinear | bicubic, border, align_corners=True)
// (warp.py:92-116, 325-343).  Same float32 operation sequence as oracle/cc_oracle.c section 11 (the canon of the
// reference run: fused linspace, plain weight products + fma accumulation for bilinear, the mixed plain / fused
// evaluation of the bicubic coefficients and sums).
__device__ __forceinline__ float ic_lin_coord(int i, int n) {
    if (n == 1) return -1.0f;
    const float step = __fdiv_rn(2.0f, static_cast<float>(n - 1));
    return i < n / 2 ? __fmaf_rn(step, static_cast<float>(i), -1.0f) : __fmaf_rn(-step, static_cast<float>(n - 1 - i), 1.0f);
}
__device__ __forceinline__ float ic_cubic_inner(float x) {
    const float A = -0.75f;
    const float t = __fmul_rn(__fmaf_rn(A + 2.0f, x, -(A + 3.0f)), x);
    return __fmaf_rn(t, x, 1.0f);
}
__device__ __forceinline__ float ic_cubic_outer(float x) {
    const float A = -0.75f;
    float t = __fmul_rn(A, x);
    t = __fsub_rn(t, 5.0f * A);
    t = __fmul_rn(t, x);
    t = __fadd_rn(t, 8.0f * A);
    t = __fmul_rn(t, x);
    return __fsub_rn(t, 4.0f * A);
}
// the position, in samples, that sample i of an axis of n reads under the flow f (normalised and back, as grid_sample does)
__device__ __forceinline__ float ic_native_coord(float f, int i, int n) {
    const float s = static_cast<float>((n - 1.0) / 2.0);
    const float g = __fadd_rn(ic_lin_coord(i, n), __fdiv_rn(f, s));
    return __fmul_rn(__fadd_rn(g, 1.0f), s);
}
// bilinear: the position is clamped to the picture (in place); the floor of the position
__device__ __forceinline__ float ic_native_floor(int n_taps, float& c, int n) {
    if (n_taps == 2) c = fminf(static_cast<float>(n - 1), fmaxf(c, 0.0f));
    return floorf(c);
}
// ... and from it the position of tap j of the window (2 taps from the floor, 4 from one before it; the floor saturated)
__device__ __forceinline__ int ic_native_tap(int n_taps, float c0f, int n, int j) {
    if (n_taps == 2) return static_cast<int>(c0f) + j;
    return static_cast<int>(fminf(fmaxf(c0f, -4.0f), static_cast<float>(n) + 4.0f)) - 1 + j;
}
__device__ __forceinline__ void ic_warp_pixel_native(const float* __restrict__ ref, int H, int W, int gx, int gy, int n_taps, float fx,
                                                     float fy, int y, int x, float out[3]) {
    float ix = ic_native_coord(fx, x, W), iy = ic_native_coord(fy, y, H);
    const size_t plane = static_cast<size_t>(H) * W;
    if (n_taps == 2) {
        const float x0f = ic_native_floor(2, ix, W), y0f = ic_native_floor(2, iy, H);
        const float w = __fsub_rn(ix, x0f), e = __fsub_rn(1.0f, w), n = __fsub_rn(iy, y0f), s = __fsub_rn(1.0f, n);
        const float w_nw = __fmul_rn(s, e), w_ne = __fmul_rn(s, w), w_sw = __fmul_rn(n, e), w_se = __fmul_rn(n, w);
        const int xa = ic_tap_index(ic_native_tap(2, x0f, W, 0), W, gx), xb = ic_tap_index(ic_native_tap(2, x0f, W, 1), W, gx);
        const int ya = ic_tap_index(ic_native_tap(2, y0f, H, 0), H, gy), yb = ic_tap_index(ic_native_tap(2, y0f, H, 1), H, gy);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* r = ref + c * plane;
            float acc = __fmul_rn(r[static_cast<size_t>(ya) * W + xa], w_nw);
            acc = __fmaf_rn(r[static_cast<size_t>(ya) * W + xb], w_ne, acc);
            acc = __fmaf_rn(r[static_cast<size_t>(yb) * W + xa], w_sw, acc);
            acc = __fmaf_rn(r[static_cast<size_t>(yb) * W + xb], w_se, acc);
            out[c] = acc;
        }
        return;
    }
    const float x0f = ic_native_floor(4, ix, W), y0f = ic_native_floor(4, iy, H);
    const float tx = __fsub_rn(ix, x0f), ty = __fsub_rn(iy, y0f);
    const float cx[4] = {ic_cubic_outer(__fadd_rn(tx, 1.0f)), ic_cubic_inner(tx), ic_cubic_inner(__fsub_rn(1.0f, tx)), ic_cubic_outer(__fsub_rn(2.0f, tx))};
    const float cy[4] = {ic_cubic_outer(__fadd_rn(ty, 1.0f)), ic_cubic_inner(ty), ic_cubic_inner(__fsub_rn(1.0f, ty)), ic_cubic_outer(__fsub_rn(2.0f, ty))};
    int xs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xs[j] = ic_tap_index(ic_native_tap(4, x0f, W, j), W, gx);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float row[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int yy = ic_tap_index(ic_native_tap(4, y0f, H, i), H, gy);
            const float* r = ref + c * plane + static_cast<size_t>(yy) * W;
            float acc = __fmaf_rn(r[xs[0]], cx[0], __fmul_rn(r[xs[1]], cx[1]));
            acc = __fadd_rn(acc, __fmul_rn(r[xs[2]], cx[2]));
            acc = __fadd_rn(acc, __fmul_rn(r[xs[3]], cx[3]));
            row[i] = acc;
        }
        float acc = __fmaf_rn(row[1], cy[1], __fmul_rn(row[0], cy[0]));
        acc = __fmaf_rn(row[2], cy[2], acc);
        acc = __fmaf_rn(row[3], cy[3], acc);
        out[c] = acc;
    }
}

// one reference warped to pixel (y, x).  NT = 8: the sinc-8 warp of every preset; NT = 0: a run-time tap count - the native path for
// 2 / 4 taps, the sinc warp for any even size from 6
template <int NT>
__device__ __forceinline__ void ic_warp(const float* __restrict__ ref, int H, int W, int gx, int gy, int n_taps, float fx, float fy, int y, int x,
                                        float out[3]) {
    if (NT == 0 && n_taps < 6) return ic_warp_pixel_native(ref, H, W, gx, gy, n_taps, fx, fy, y, x, out);
    const float rxf = floorf(fx), ryf = floorf(fy);
    const float sx = fx - rxf, sy = fy - ryf;
    float cx[kTapCap<NT>], cy[kTapCap<NT>];
    ic_coeffs<NT>(sx, n_taps, cx);
    ic_coeffs<NT>(sy, n_taps, cy);
    ic_taps<NT>(ref, H, W, gx, gy, n_taps, ic_tap_offset(rxf, W), ic_tap_offset(ryf, H), cx, cy, y, x, out);
}

// the interval [a, b] of reference indices that ic_warp<NT> reads along one axis (n samples, global shift g) for sample i with
// the flow f: the first tap from the pieces the warps use, then ic_tap_index of the two ends
template <int NT>
__device__ __forceinline__ void ic_window_axis(int n_taps, float f, int i, int n, int g, int& a, int& b) {
    const int nt = NT > 0 ? NT : n_taps;
    int first;
    if (NT == 0 && n_taps < 6) {
        float c = ic_native_coord(f, i, n);
        const float c0f = ic_native_floor(n_taps, c, n);
        first = ic_native_tap(n_taps, c0f, n, 0);
    } else {
        first = ic_sinc_tap(i, nt, 0, ic_tap_offset(floorf(f), n));
    }
    a = ic_tap_index(first, n, g);
    b = ic_tap_index(first + nt - 1, n, g);
}

// ---- the blend (decode.py:170-189): weight = clamp(alpha | beta + 0.5, 0, 1), prediction = beta w0 + (1 - beta) w1 (B frames),
// sample = alpha prediction + residue.  Every multiply and every add is an operation of its own, never an fma: bit parity with
// oracle/cc_oracle.c section 11.
__device__ __forceinline__ float ic_weight(float v) { const float a = v + 0.5f; return a < 0.0f ? 0.0f : (a > 1.0f ? 1.0f : a); }
__device__ __forceinline__ float ic_mix(float b, float w0, float w1) { const float t0 = b * w0, t1 = (1.0f - b) * w1; return t0 + t1; }
__device__ __forceinline__ float ic_sample(float a, float pred, float residue) { const float m = a * pred; return m + residue; }
// the tail of inter_recon_body for the unit walk (di_pixel): sample i from its warped references (w1: B frames) and a = ic_weight(alpha)
__device__ __forceinline__ void ic_blend(bool two, const float* __restrict__ residue, size_t plane, size_t i, float a, const float w0[3],
                                         const float w1[3], float out[3]) {
    float pred[3];
    if (two) {
        const float b = ic_weight(residue[4 * plane + i]);
#pragma unroll
        for (int c = 0; c < 3; ++c) pred[c] = ic_mix(b, w0[c], w1[c]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) pred[c] = w0[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = ic_sample(a, pred[c], residue[c * plane + i]);
}

struct InterParams {
    const float* residue;  // [4 | 5][H][W]
    const float* motion;   // [2 | 4][H][W]
    const float* ref0;     // [3][H][W]
    const float* ref1;     // B frames
    float* out;            // [3][H][W]
    int frame_type, H, W, n_taps;
    int gflow[4];
};
static InterParams inter_params(int frame_type, int h, int w, int n_taps, const int* gflow, const float* residue, const float* motion,
                                const float* ref0, const float* ref1, float* out) {
    InterParams p;
    p.residue = residue; p.motion = motion; p.ref0 = ref0; p.ref1 = ref1; p.out = out;
    p.frame_type = frame_type; p.H = h; p.W = w; p.n_taps = n_taps;
    for (int i = 0; i < 4; ++i) p.gflow[i] = gflow[i];
    return p;
}

// ---- r06: the warp's coefficients ahead of the references.  A frame's flows (the motion cool-chic's output) are known long before
// its references are: in a hierarchical GOP every B-frame cool-chic is decoded at ~0.5 of the I frames' chains (fewer symbols), and
// everything then waits for the I frames.  The f64 sin / cos of the sinc window - 64 evaluations per pixel and reference pair - only
// depend on the flows, so ccd_decode_video CAN compute them in that gap (CCD_VIDEO_COEF_MB: inter_coef8_kernel, 16 coefficients per
// pixel and reference, 64 B) and only gather behind the references (inter_apply8_kernel).  Same functions, same operation order:
// bit-identical to the one-kernel form.  Measured: the gather alone is 0.26 of the 0.34 ms - off by default (ccd_video.cpp).
// coef layout: float4 [ref][4][H * W] - quad 0 / 1 = cx[0..3] / cx[4..7], quad 2 / 3 = cy: every access a coalesced 16 bytes per lane.
__global__ __launch_bounds__(256) void inter_coef8_kernel(const float* __restrict__ motion, int H, int W, int n_refs, float4* __restrict__ coef) {
    int x, y;
    tile_pixel(blockIdx.x, blockIdx.y, &x, &y);
    if (x >= W || y >= H) return;
    const size_t plane = static_cast<size_t>(H) * W, i = static_cast<size_t>(y) * W + x;
    for (int r = 0; r < n_refs; ++r) {
        const float fx = motion[(2 * r) * plane + i], fy = motion[(2 * r + 1) * plane + i];
        const float sx = fx - floorf(fx), sy = fy - floorf(fy);
        float cx[8], cy[8];
        ic_coeffs<8>(sx, 8, cx);
        ic_coeffs<8>(sy, 8, cy);
        float4* o = coef + static_cast<size_t>(r) * 4 * plane + i;
        o[0] = make_float4(cx[0], cx[1], cx[2], cx[3]);
        o[plane] = make_float4(cx[4], cx[5], cx[6], cx[7]);
        o[2 * plane] = make_float4(cy[0], cy[1], cy[2], cy[3]);
        o[3 * plane] = make_float4(cy[4], cy[5], cy[6], cy[7]);
    }
}
__device__ __forceinline__ void ic_warp_pixel_coef8(const float* __restrict__ ref, const float4* __restrict__ coef, size_t plane, size_t i, int H, int W, int gx,
                                                    int gy, float fx, float fy, int y, int x, float out[3]) {
    const float4 a = coef[i], b = coef[plane + i], c = coef[2 * plane + i], d = coef[3 * plane + i];
    const float cx[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, cy[8] = {c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
    ic_taps<8>(ref, H, W, gx, gy, 8, ic_tap_offset(floorf(fx), W), ic_tap_offset(floorf(fy), H), cx, cy, y, x, out);
}

// reference r of the frame warped to pixel (y, x); AHEAD: the sinc-8 coefficients come from the `coef` block
template <int NT, bool AHEAD>
__device__ __forceinline__ void inter_warp_ref(const InterParams& p, const float4* __restrict__ coef, int r, size_t plane, size_t i, int y, int x,
                                               float out[3]) {
    const float* ref = r ? p.ref1 : p.ref0;
    const float fx = p.motion[(2 * r) * plane + i], fy = p.motion[(2 * r + 1) * plane + i];
    if constexpr (AHEAD) ic_warp_pixel_coef8(ref, coef + static_cast<size_t>(r) * 4 * plane, plane, i, p.H, p.W, p.gflow[2 * r], p.gflow[2 * r + 1], fx, fy, y, x, out);
    else ic_warp<NT>(ref, p.H, p.W, p.gflow[2 * r], p.gflow[2 * r + 1], p.n_taps, fx, fy, y, x, out);
}
// One pixel of a P / B frame.  The mix stays inside the B branch, behind the second warp: hoisted behind both warps, the 8-tap
// kernels need 256 registers and run one wave per SIMD - and through ic_blend, which sits behind both, inter_recon_kernel<8> needs
// 206 and runs two, so the tail is written out here.
template <int NT, bool AHEAD>
__device__ __forceinline__ void inter_recon_body(const InterParams& p, const float4* __restrict__ coef) {
    int x, y;
    tile_pixel(blockIdx.x, blockIdx.y, &x, &y);
    if (x >= p.W || y >= p.H) return;
    const size_t plane = static_cast<size_t>(p.H) * p.W, i = static_cast<size_t>(y) * p.W + x;
    const float a = ic_weight(p.residue[3 * plane + i]);
    float w0[3], pred[3];
    inter_warp_ref<NT, AHEAD>(p, coef, 0, plane, i, y, x, w0);
    if (p.frame_type == 2) {
        const float b = ic_weight(p.residue[4 * plane + i]);
        float w1[3];
        inter_warp_ref<NT, AHEAD>(p, coef, 1, plane, i, y, x, w1);
#pragma unroll
        for (int c = 0; c < 3; ++c) pred[c] = ic_mix(b, w0[c], w1[c]);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) pred[c] = w0[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) p.out[c * plane + i] = ic_sample(a, pred[c], p.residue[c * plane + i]);
}
template <int NT>  // 0: run-time tap count (any even size, and the native 2- / 4-tap paths); 8: the sinc-8 warp of every preset
__global__ __launch_bounds__(256) void inter_recon_kernel(InterParams p) { inter_recon_body<NT, false>(p, nullptr); }
__global__ __launch_bounds__(256) void inter_apply8_kernel(InterParams p, const float4* __restrict__ coef) { inter_recon_body<8, true>(p, coef); }

size_t inter_coef_bytes(int frame_type, int h, int w) { return static_cast<size_t>(frame_type == 2 ? 2 : 1) * 4 * h * w * sizeof(float4); }
hipError_t launch_inter_coef8(int frame_type, int h, int w, const float* motion, void* coef, hipStream_t stream) {
    hipLaunchKernelGGL(inter_coef8_kernel, tile_grid(h, w), dim3(256), 0, stream, motion, h, w, frame_type == 2 ? 2 : 1, static_cast<float4*>(coef));
    return hipGetLastError();
}
hipError_t launch_inter_apply8(int frame_type, int h, int w, const int* gflow, const float* residue, const float* motion, const float* ref0,
                               const float* ref1, const void* coef, float* out, hipStream_t stream) {
    const InterParams p = inter_params(frame_type, h, w, 8, gflow, residue, motion, ref0, ref1, out);
    hipLaunchKernelGGL(inter_apply8_kernel, tile_grid(h, w), dim3(256), 0, stream, p, static_cast<const float4*>(coef));
    return hipGetLastError();
}
hipError_t launch_inter_recon(int frame_type, int h, int w, int n_taps, const int* gflow, const float* residue, const float* motion,
                              const float* ref0, const float* ref1, float* out, hipStream_t stream) {
    const InterParams p = inter_params(frame_type, h, w, n_taps, gflow, residue, motion, ref0, ref1, out);
    if (n_taps == 8) hipLaunchKernelGGL(inter_recon_kernel<8>, tile_grid(h, w), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(inter_recon_kernel<0>, tile_grid(h, w), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// ---- P / B frames by units: the walk that dsens_inter_kernel, dsens_dep_kernel and inter_score_kernel share (DESIGN.md 4.15, 4.16,
// 4.19; the job: InterUnitJob, ccd_device.hpp).  A job is one frame to reconstruct; its workgroups find it in a prefix table
// (di_locate), a thread owns one unit: one luma sample or, 4:2:0, one 2 x 2 quad and its chroma sample.  Per sample (di_unit) the
// operations of inter_recon_kernel (same device functions: ic_warp and ic_blend) followed by those of planes_kernel (ccd_float.hip;
// the sample helpers are shared, ccd_planes.hpp: round to the bit-depth grid, clamp, round; 4:2:0 chroma = the sequential f32 sum
// of the quad's rounded samples, then quantise_chroma420): the f32 that inter_recon_kernel stores and planes_kernel loads is the
// register in between, so the quantised samples are the planes of ccd_inter_reconstruct bit for bit.  What a residue candidate
// cannot change - the warped references - is computed by the base job (mode 0), kept as f32 and only read by residue jobs (mode 1);
// a motion job (mode 2) warps.  A job whose ref0 / ref1 are OTHER planes than the frame's references (a reference item, DESIGN.md
// 4.22) is a mode 2 job where all of the frame's references are replaced, and mode 3 / 4 where only reference 0 / 1 of a B frame
// is: that one is warped, the other's kept warp is read.  What becomes of a quantised sample is the kernel's sink.
__device__ __forceinline__ void di_store(void* plane, size_t at, unsigned v, int wide) {
    if (wide) static_cast<uint16_t*>(plane)[at] = static_cast<uint16_t>(v);
    else static_cast<uint8_t*>(plane)[at] = static_cast<uint8_t>(v);
}

// the frame's float sample (y, x) of the three channels: what inter_recon_body stores, from the same pieces
template <int NT>
__device__ __forceinline__ void di_pixel(const InterUnitJob& J, int y, int x, float out[3]) {
    const size_t plane = static_cast<size_t>(J.H) * J.W, i = static_cast<size_t>(y) * J.W + x;
    const float a = ic_weight(J.residue[3 * plane + i]);
    const bool two = J.frame_type == 2;
    float w0[3] = {0.0f, 0.0f, 0.0f}, w1[3] = {0.0f, 0.0f, 0.0f};
    if (J.mode == 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { w0[c] = J.w0[c * plane + i]; if (two) w1[c] = J.w1[c * plane + i]; }
    } else {
        // one body for both references (the straight-line f64 evaluations of two inlined warps cost twice the registers); the
        // selects keep w0 / w1 out of indexed private memory
        const int n_refs = two ? 2 : 1;
        // a reference item with one reference of a B frame replaced (mode 3 / 4) warps that one and reads the other's kept warp
        const int kept = J.mode == 3 ? 1 : (J.mode == 4 ? 0 : -1);
#pragma unroll 1
        for (int r = 0; r < n_refs; ++r) {
            float w[3];
            if (r == kept) {
                const float* k = r ? J.w1 : J.w0;
#pragma unroll
                for (int c = 0; c < 3; ++c) w[c] = k[c * plane + i];
            } else {
                ic_warp<NT>(r ? J.ref1 : J.ref0, J.H, J.W, r ? J.gflow[2] : J.gflow[0], r ? J.gflow[3] : J.gflow[1], J.n_taps,
                            J.motion[(2 * r) * plane + i], J.motion[(2 * r + 1) * plane + i], y, x, w);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) { w0[c] = r == 0 ? w[c] : w0[c]; w1[c] = r == 1 ? w[c] : w1[c]; }
        }
        if (J.mode == 0 && J.w0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { J.w0[c * plane + i] = w0[c]; if (two) J.w1[c * plane + i] = w1[c]; }
        }
    }
    ic_blend(two, J.residue, plane, i, a, w0, w1, out);
}

// The job of this workgroup, its index `local` among the job's workgroups and the thread's unit; `inside`: the unit lies inside the
// frame (a flag, not a return: inter_score_kernel's threads all meet at a barrier).
struct DiUnit { uint32_t local; int ux, uy; bool inside; };
template <class Job>
__device__ __forceinline__ const Job& di_locate(const Job* __restrict__ jobs, const uint32_t* __restrict__ prefix, int n_jobs, DiUnit& u) {
    const uint32_t blk = blockIdx.x;
    const int j = entry_of(prefix, n_jobs, blk);
    const InterUnitJob& J = unit_job(jobs[j]);  // (uniform: scalar loads)
    u.local = blk - prefix[j];
    const uint32_t tiles_x = static_cast<uint32_t>(J.tiles_x);
    tile_pixel(u.local % tiles_x, u.local / tiles_x, &u.ux, &u.uy);
    u.inside = u.ux < (J.W >> J.chroma_shift) && u.uy < (J.H >> J.chroma_shift);  // (4:2:0 frames have even sides)
    return jobs[j];
}
// Unit (ux, uy) of the frame: sink(plane, index, quantised sample) once per output sample - 4:4:4 the three planes at i; 4:2:0 the
// four luma samples, then the two chroma samples at ci.
template <int NT, class Sink>
__device__ __forceinline__ void di_unit(const InterUnitJob& J, int ux, int uy, Sink&& sink) {
    const int cs = J.chroma_shift;
    const float maxv = J.maxv;
    float v[3], sum1 = 0.0f, sum2 = 0.0f;  // planes_kernel's order over the quad: dy outer, dx inner
    const int n = cs ? 4 : 1;              // one loop body for both shapes: the warp is instantiated once
#pragma unroll 1
    for (int q = 0; q < n; ++q) {
        const int y = (uy << cs) + (q >> 1), x = (ux << cs) + (q & 1);
        di_pixel<NT>(J, y, x, v);
        const size_t i = static_cast<size_t>(y) * J.W + x;
        sink(0, i, quantise_sample(v[0], maxv));
        if (!cs) {
            sink(1, i, quantise_sample(v[1], maxv));
            sink(2, i, quantise_sample(v[2], maxv));
        } else {
            sum1 += round_to_grid(v[1], maxv);
            sum2 += round_to_grid(v[2], maxv);
        }
    }
    if (!cs) return;
    const size_t ci = static_cast<size_t>(uy) * (J.W / 2) + ux;
    sink(1, ci, quantise_chroma420(sum1, maxv));
    sink(2, ci, quantise_chroma420(sum2, maxv));
}
// One launch over jobs and their prefix table of workgroups: the sinc-8 instantiation or the run-time one; nothing when empty.
template <class Job, class... X>
static hipError_t launch_jobs(void (*k8)(const Job*, const uint32_t*, int, X...), void (*k0)(const Job*, const uint32_t*, int, X...), unsigned threads,
                              const Job* d_jobs, const uint32_t* d_prefix, int n_jobs, uint32_t n_blocks, int sinc8, hipStream_t stream, X... extra) {
    if (n_jobs <= 0 || n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(sinc8 ? k8 : k0, dim3(n_blocks), dim3(threads), 0, stream, d_jobs, d_prefix, n_jobs, extra...);
    return hipGetLastError();
}

// ---- distortion deltas of P / B frames (ccd_dsens_add_inter): the integer planes of every probe slot of a round in
// one launch.  A job is one slot.  Every output word has one writer.  Plain vector stores; no atomics, no waits, no LDS.
template <int NT>  // as inter_recon_kernel: 8 = the sinc-8 warp of every preset, 0 = a run-time tap count and the native paths
__global__ __launch_bounds__(256) void dsens_inter_kernel(const InterUnitJob* __restrict__ jobs, const uint32_t* __restrict__ prefix, int n_jobs) {
    DiUnit u;
    const InterUnitJob J = di_locate(jobs, prefix, n_jobs, u);  // (a copy: scalar registers)
    if (!u.inside) return;
    di_unit<NT>(J, u.ux, u.uy, [&](int p, size_t at, unsigned q) { di_store(J.plane[p], at, q, J.wide); });
}
hipError_t launch_dsens_inter(const InterUnitJob* d_jobs, const uint32_t* d_prefix, int n_jobs, uint32_t n_blocks, int sinc8, hipStream_t stream) {
    return launch_jobs(dsens_inter_kernel<8>, dsens_inter_kernel<0>, 256, d_jobs, d_prefix, n_jobs, n_blocks, sinc8, stream);
}

// ---- distortion deltas through the frames that predict from a moved one (ccd_dsens_add_dependent).  A job is one
// (candidate, dependent, probe slot) of a round: the dependent frame F reconstructed with the candidate's PROBE planes as its
// reference `which`.  The warp is not pointwise in the reference: a sample of F reads an N x N window at a flow-displaced place,
// so the change of one latent of the reference scatters into F wherever F's flows point.  Per unit (one luma sample, or one 4:2:0
// quad and its chroma sample; the tiles of dsens_inter_kernel):
//   (a) the interval of reference indices every sample's window reads, per axis (ic_window_axis: the warps' own index pieces);
//   (b) lattice_hit (ccd_lattice.hpp) on both axes: which members of the pass's lattice have their reference-change region under
//       a window.  None: the unit reads unchanged reference samples only and is F's base, bit for bit - done.  Exactly one: the
//       unit is reconstructed with the functions of dsens_inter_kernel and quantised, and the sum over its samples of
//       (F' - src)^2 - (F - src)^2 goes to that entry's accumulator with one 64-bit integer atomic add (any order, same bits);
//   (c) more than one: a conflict - the unit's change cannot be split between the entries, so each entry hit gets the byte 1 in
//       `flag` (plain stores; every writer stores the same value) and dsens_dep_final_kernel turns it into the sentinel.
// Only DIRECT dependents: frames that predict from F are not followed.  No LDS, no waits, no spinning.
__device__ __forceinline__ int di_load(const void* plane, size_t at, int wide) {
    return wide ? static_cast<int>(static_cast<const uint16_t*>(plane)[at]) : static_cast<int>(static_cast<const uint8_t*>(plane)[at]);
}
__device__ __forceinline__ long long di_gain(int q, int base, int src) {
    const long long dq = q - src, db = base - src;
    return dq * dq - db * db;
}
// what the windows of sample (y, x) hit: counts per axis (0 on either: nothing) and the first member of each
template <int NT>
__device__ __forceinline__ bool dd_sample_hits(const DsensDepJob& D, int y, int x, int& fy, int& cy, int& fx, int& cx) {
    const InterUnitJob& J = D.recon;
    const size_t plane = static_cast<size_t>(J.H) * J.W, i = static_cast<size_t>(y) * J.W + x;
    const int r = D.which;
    int a, b;
    ic_window_axis<NT>(J.n_taps, J.motion[(2 * r + 1) * plane + i], y, J.H, r ? J.gflow[3] : J.gflow[1], a, b);
    cy = lattice_hit(D.ay, D.stride, D.py, a, b, &fy);
    cx = 0;
    if (cy == 0) return false;
    ic_window_axis<NT>(J.n_taps, J.motion[(2 * r) * plane + i], x, J.W, r ? J.gflow[2] : J.gflow[0], a, b);
    cx = lattice_hit(D.ax, D.stride, D.px, a, b, &fx);
    return cx != 0;
}

template <int NT>
__global__ __launch_bounds__(256) void dsens_dep_kernel(const DsensDepJob* __restrict__ jobs, const uint32_t* __restrict__ prefix, int n_jobs) {
    DiUnit u;
    const DsensDepJob& D = di_locate(jobs, prefix, n_jobs, u);
    if (!u.inside) return;
    const InterUnitJob& J = D.recon;
    const int ux = u.ux, uy = u.uy;
    const int cs = J.chroma_shift, n = cs ? 4 : 1;
    const size_t map_plane = D.move > 0 ? static_cast<size_t>(D.h) * D.w : 0;
    int state = 0, ey = 0, ex = 0;  // 0: nothing hit, 1: the entry (ey, ex) alone, 2: a conflict
#pragma unroll 1
    for (int q = 0; q < n; ++q) {
        int fy, cy, fx, cx;
        if (!dd_sample_hits<NT>(D, (uy << cs) + (q >> 1), (ux << cs) + (q & 1), fy, cy, fx, cx)) continue;
        if (cy > 1 || cx > 1 || (state == 1 && (fy != ey || fx != ex))) state = 2;
        else if (state == 0) { state = 1; ey = fy; ex = fx; }
    }
    if (state == 0) return;
    if (state == 2) {
#pragma unroll 1
        for (int q = 0; q < n; ++q) {
            int fy, cy, fx, cx;
            if (!dd_sample_hits<NT>(D, (uy << cs) + (q >> 1), (ux << cs) + (q & 1), fy, cy, fx, cx)) continue;
            for (int iy = 0; iy < cy; ++iy)
                for (int ix = 0; ix < cx; ++ix)
                    D.flag[map_plane + static_cast<size_t>(fy + iy * D.stride) * D.w + (fx + ix * D.stride)] = 1;
        }
        return;
    }
    long long gain = 0;
    di_unit<NT>(J, ux, uy, [&](int p, size_t at, unsigned q) {
        gain += di_gain(static_cast<int>(q), di_load(J.plane[p], at, J.wide), di_load(D.src[p], at, J.wide));
    });
    if (gain != 0) atomicAdd(D.acc + map_plane + static_cast<size_t>(ey) * D.w + ex, static_cast<unsigned long long>(gain));
}

hipError_t launch_dsens_dep(const DsensDepJob* d_jobs, const uint32_t* d_prefix, int n_jobs, uint32_t n_blocks, int sinc8, hipStream_t stream) {
    return launch_jobs(dsens_dep_kernel<8>, dsens_dep_kernel<0>, 256, d_jobs, d_prefix, n_jobs, n_blocks, sinc8, stream);
}

// ---- the squared error of many candidates of P / B frames in one launch (ccd_iscore).  A job is one candidate of
// one frame: the frame's two float outputs with one of them replaced.  The unit walk with a sink that takes (sample - source)^2, as
// integers, so the sums are those of ccd_inter_reconstruct followed by the quality meter.  No plane is stored.  Reduction as quality_sse_kernel: u64 per lane and plane, wave shuffle, the four wave partials through LDS, one
// thread stores the workgroup's three partials; inter_score_final_kernel adds a job's partials in a fixed order.  Plain vector
// stores; no atomics, no waits on other workgroups.
__device__ __forceinline__ uint64_t is_wave_sum(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(static_cast<unsigned long long>(v), off, 64);
    return v;
}
__device__ __forceinline__ uint64_t is_sq(unsigned q, int src) {
    const int64_t d = static_cast<int64_t>(q) - src;
    return static_cast<uint64_t>(d * d);
}

template <int NT>  // as dsens_inter_kernel
__global__ __launch_bounds__(256) void inter_score_kernel(const InterScoreJob* __restrict__ jobs, const uint32_t* __restrict__ prefix, int n_jobs,
                                                          uint64_t* __restrict__ part) {
    __shared__ uint64_t wave_part[3][4];
    DiUnit u;
    const InterScoreJob& S = di_locate(jobs, prefix, n_jobs, u);
    const InterUnitJob& J = S.recon;
    uint64_t e0 = 0, e1 = 0, e2 = 0;
    if (u.inside) {  // (every thread reaches the barrier below)
        di_unit<NT>(J, u.ux, u.uy, [&](int p, size_t at, unsigned q) {
            const uint64_t e = is_sq(q, di_load(S.src[p], at, J.wide));
            if (p == 0) e0 += e; else if (p == 1) e1 += e; else e2 += e;
        });
    }
    e0 = is_wave_sum(e0); e1 = is_wave_sum(e1); e2 = is_wave_sum(e2);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) { wave_part[0][tid >> 6] = e0; wave_part[1][tid >> 6] = e1; wave_part[2][tid >> 6] = e2; }
    __syncthreads();
    if (tid == 0) {
        uint64_t* out = part + (static_cast<size_t>(S.part_first) + u.local) * 3;
#pragma unroll
        for (int p = 0; p < 3; ++p) out[p] = wave_part[p][0] + wave_part[p][1] + wave_part[p][2] + wave_part[p][3];
    }
}

// One wave per (job, plane): adds the job's workgroup partials of the plane, lane-strided, then the shuffle tree.
__global__ __launch_bounds__(64) void inter_score_final_kernel(const InterScoreRange* __restrict__ ranges, const uint64_t* __restrict__ part,
                                                               uint64_t* __restrict__ sse) {
    const uint32_t r = blockIdx.x / 3, p = blockIdx.x % 3;
    const InterScoreRange R = ranges[r];
    uint64_t acc = 0;
    for (uint32_t i = threadIdx.x; i < R.count; i += 64) acc += part[(static_cast<size_t>(R.first) + i) * 3 + p];
    acc = is_wave_sum(acc);
    if (threadIdx.x == 0) sse[static_cast<size_t>(r) * 3 + p] = acc;
}

hipError_t launch_inter_score(const InterScoreJob* d_jobs, const uint32_t* d_prefix, int n_jobs, uint32_t n_blocks, int sinc8, uint64_t* d_part,
                              hipStream_t stream) {
    return launch_jobs(inter_score_kernel<8>, inter_score_kernel<0>, 256, d_jobs, d_prefix, n_jobs, n_blocks, sinc8, stream, d_part);
}
hipError_t launch_inter_score_final(const InterScoreRange* d_ranges, int n_ranges, const uint64_t* d_part, uint64_t* d_sse, hipStream_t stream) {
    if (n_ranges <= 0) return hipSuccess;
    hipLaunchKernelGGL(inter_score_final_kernel, dim3(static_cast<uint32_t>(n_ranges) * 3), dim3(64), 0, stream, d_ranges, d_part, d_sse);
    return hipGetLastError();
}

// ---- where the samples of a dependent frame read its reference, in cells of the RDOQ claim raster (ccd_rdoq_follow; DESIGN.md
// 4.17).  A job is one follow: the dependent F's flows into its reference `which`.  A workgroup is one wave and one cell C of F,
// a lane per luma sample of the cell: (a) the interval of reference indices the sample's window reads per axis (ic_window_axis,
// as dsens_dep_kernel), (b) a wave reduction to the bounding rectangle of the cell's windows - inside the picture already, the
// indices are clamped - (c) the lanes over the reference cells c the rectangle meets: reach[c] grows to hold C, four 32-bit
// vector atomicMin per cell (the two upper bounds are kept complemented, so that all four are minima and all ones is "nobody").
// Any order of the atomics leaves the same words.  No LDS, no waits, no spinning.
template <int NT>
__global__ __launch_bounds__(64) void rdoq_reach_kernel(const RdoqReachJob* __restrict__ jobs, const uint32_t* __restrict__ prefix, int n_jobs) {
    const int j = entry_of(prefix, n_jobs, blockIdx.x);
    const RdoqReachJob& J = jobs[j];  // (uniform: scalar loads)
    const uint32_t local = blockIdx.x - prefix[j], cw = static_cast<uint32_t>(J.cells_w);
    const uint32_t Cy = local / cw, Cx = local - Cy * cw;
    if (Cy >= static_cast<uint32_t>(J.cells_h)) return;
    const uint32_t lane = threadIdx.x;
    const int y = static_cast<int>(Cy) * kRdoqCell + static_cast<int>(lane) / kRdoqCell;
    const int x = static_cast<int>(Cx) * kRdoqCell + static_cast<int>(lane) % kRdoqCell;
    int ya = INT32_MAX, yb = -1, xa = INT32_MAX, xb = -1;
    if (y < J.H && x < J.W) {  // (the sample (0, 0) of a cell always is: no cell is empty)
        const size_t plane = static_cast<size_t>(J.H) * J.W, i = static_cast<size_t>(y) * J.W + x;
        ic_window_axis<NT>(J.n_taps, J.motion[(2 * J.which + 1) * plane + i], y, J.H, J.gy, ya, yb);
        ic_window_axis<NT>(J.n_taps, J.motion[(2 * J.which) * plane + i], x, J.W, J.gx, xa, xb);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ya = min(ya, __shfl_xor(ya, off, 64)); xa = min(xa, __shfl_xor(xa, off, 64));
        yb = max(yb, __shfl_xor(yb, off, 64)); xb = max(xb, __shfl_xor(xb, off, 64));
    }
    if (yb < ya || xb < xa) return;
    // the indices are ic_tap_index's, inside [0, n - 1]; the bounds of the table are this kernel's to keep all the same
    const uint32_t top = min(static_cast<uint32_t>(max(ya, 0) / kRdoqCell), static_cast<uint32_t>(J.cells_h - 1));
    const uint32_t left = min(static_cast<uint32_t>(max(xa, 0) / kRdoqCell), cw - 1);
    const uint32_t bottom = min(static_cast<uint32_t>(yb / kRdoqCell), static_cast<uint32_t>(J.cells_h - 1));
    const uint32_t right = min(static_cast<uint32_t>(xb / kRdoqCell), cw - 1);
    const uint32_t bw = right - left + 1, n = (bottom - top + 1) * bw;
    for (uint32_t t = lane; t < n; t += 64) {
        const uint32_t r = t / bw, q = t - r * bw;
        uint32_t* w = J.reach + (static_cast<size_t>(top + r) * cw + left + q) * kRdoqReachWords;
        atomicMin(w, Cy);
        atomicMin(w + 1, Cx);
        atomicMin(w + 2, ~Cy);
        atomicMin(w + 3, ~Cx);
    }
}

hipError_t launch_rdoq_reach(const RdoqReachJob* d_jobs, const uint32_t* d_prefix, int n_jobs, uint32_t n_blocks, int sinc8, hipStream_t stream) {
    return launch_jobs(rdoq_reach_kernel<8>, rdoq_reach_kernel<0>, 64, d_jobs, d_prefix, n_jobs, n_blocks, sinc8, stream);
}

// ---- a kernel that only takes time: ccd_runtime.cpp measures with it which of the library's side streams run concurrently
__global__ void spin_kernel(unsigned long long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    while (__builtin_amdgcn_s_memtime() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
hipError_t launch_spin(unsigned long long ticks, hipStream_t stream) {
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, stream, ticks);
    return hipGetLastError();
}

}  // namespace ccd
