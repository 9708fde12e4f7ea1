// ccd_quality.hip - PSNR and MS-SSIM of decoded integer planes against their source, on the device (gfx950).
//
// Three kernels score every plane of every item of a batch.  Work is cut into tiles and a workgroup finds the plane of its
// tile in a prefix table (as the PNG packer's blocks do), so small and large pictures share the launches.
//   quality_sse_kernel     one tile = kQSseBytes of both pictures: 16-byte loads, u64 sums per lane, one partial per workgroup.
//   quality_msssim_kernel  launched once per scale.  One tile = 32 x 32 window positions: both pictures' 42 x 42 samples are
//                          staged in LDS, the separable 11-tap pass runs for the five moment maps (x, y, x^2, y^2, xy), cs and
//                          ssim are formed per pixel and summed over the tile.  The same workgroup writes the 2 x 2 pooled
//                          pictures of the next scale from its staged samples: those are the only intermediates in HBM.
//   quality_final_kernel   one wave per (plane, sum): adds the tile partials of the plane in a fixed order.
//
// Numbers.  The staged values are integers (scale 0: the samples; scale j: the sum of the 4^j samples under the pixel, below
// 2^24, exact as float32), the window pass accumulates them in float64 and the normalisation 1 / (maxv 4^j) is applied to the
// finished moments.  Products of two 24-bit integers are exact in float64, so the variance subtraction
// g*(x^2) - (g*x)^2 - the cancellation that limits a float32 evaluation on flat pictures - sees operands that are good to
// 2^-52.  The vector float64 rate of the CDNA4 CU is half its float32 rate and the kernel is bound by neither.
// Every float sum has a fixed order that depends on the plane alone (tile partials in a slab, then lane-strided +
// shuffle tree): no float atomics, and a picture's result does not depend on the rest of the batch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ccd_device.hpp"
#include "ccd_quality.hpp"

namespace ccd {
namespace {

constexpr int kThreads = 256;
constexpr int kSX = kQStage + 1;   // row stride of the staged samples (floats): odd, so a column walk spreads over the banks
constexpr int kHS = kQTile + 1;    // row stride of the horizontally filtered maps (doubles)

__device__ __forceinline__ uint32_t sq_diff_u8x4(uint32_t a, uint32_t b) {
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = static_cast<int>((a >> (8 * k)) & 0xffu) - static_cast<int>((b >> (8 * k)) & 0xffu);
        s += static_cast<uint32_t>(d * d);
    }
    return s;  // <= 4 * 255^2
}

__device__ __forceinline__ uint64_t sq_diff_u16x2(uint32_t a, uint32_t b) {
    const int64_t d0 = static_cast<int64_t>(a & 0xffffu) - static_cast<int64_t>(b & 0xffffu);
    const int64_t d1 = static_cast<int64_t>(a >> 16) - static_cast<int64_t>(b >> 16);
    return static_cast<uint64_t>(d0 * d0) + static_cast<uint64_t>(d1 * d1);
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(static_cast<unsigned long long>(v), off, 64);
    return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {  // fixed tree: the same operands give the same bits
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__global__ __launch_bounds__(kThreads) void quality_sse_kernel(QualityBatch B) {
    __shared__ uint64_t wave_part[kThreads / 64];
    const uint32_t tile = blockIdx.x;
    const int p = entry_of(B.sse_prefix, B.n_planes, tile);
    const QualityPlane& P = B.planes[p];
    const int wide = P.wide;
    const size_t bytes = (static_cast<size_t>(P.h) * static_cast<size_t>(P.w)) << wide;
    const size_t b0 = static_cast<size_t>(tile - B.sse_prefix[p]) * kQSseBytes;
    const size_t b1 = b0 + kQSseBytes < bytes ? b0 + kQSseBytes : bytes;
    const uint8_t* a8 = static_cast<const uint8_t*>(P.dec);
    const uint8_t* s8 = static_cast<const uint8_t*>(P.src);
    const int tid = threadIdx.x;
    uint64_t acc = 0;
    size_t done = b0;  // bytes below `done` are summed by the 16-byte loop
    if (((reinterpret_cast<uintptr_t>(a8) | reinterpret_cast<uintptr_t>(s8)) & 15u) == 0) {
        done = b1 & ~static_cast<size_t>(15);  // b0 is a multiple of 16
        for (size_t off = b0 + static_cast<size_t>(tid) * 16; off < done; off += kThreads * 16) {
            const uint4 a = *reinterpret_cast<const uint4*>(a8 + off);
            const uint4 s = *reinterpret_cast<const uint4*>(s8 + off);
            if (wide) acc += sq_diff_u16x2(a.x, s.x) + sq_diff_u16x2(a.y, s.y) + sq_diff_u16x2(a.z, s.z) + sq_diff_u16x2(a.w, s.w);
            else acc += sq_diff_u8x4(a.x, s.x) + sq_diff_u8x4(a.y, s.y) + sq_diff_u8x4(a.z, s.z) + sq_diff_u8x4(a.w, s.w);
        }
    }
    // what the wide loop left: the last partial 16 bytes of a plane, or everything of a plane that is not 16-byte aligned
    if (wide) {
        const uint16_t* a16 = static_cast<const uint16_t*>(P.dec);
        const uint16_t* s16 = static_cast<const uint16_t*>(P.src);
        for (size_t i = (done >> 1) + tid; i < (b1 >> 1); i += kThreads) {
            const int64_t d = static_cast<int64_t>(a16[i]) - static_cast<int64_t>(s16[i]);
            acc += static_cast<uint64_t>(d * d);
        }
    } else {
        for (size_t i = done + tid; i < b1; i += kThreads) {
            const int d = static_cast<int>(a8[i]) - static_cast<int>(s8[i]);
            acc += static_cast<uint64_t>(d * d);
        }
    }
    acc = wave_sum_u64(acc);
    if ((tid & 63) == 0) wave_part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) B.sse_part[tile] = wave_part[0] + wave_part[1] + wave_part[2] + wave_part[3];
}

__device__ __forceinline__ float load_sample(const void* base, int kind, size_t i) {
    if (kind == 0) return static_cast<float>(static_cast<const uint8_t*>(base)[i]);
    if (kind == 1) return static_cast<float>(static_cast<const uint16_t*>(base)[i]);
    return static_cast<const float*>(base)[i];
}

__global__ __launch_bounds__(kThreads) void quality_msssim_kernel(QualityBatch B, int scale) {
    __shared__ float sx[kQStage * kSX], sy[kQStage * kSX];
    __shared__ double hm[5][kQStage * kHS];
    __shared__ double wave_part[2][kThreads / 64];
    const uint32_t* prefix = B.ms_prefix + static_cast<size_t>(scale) * (B.n_planes + 1);
    const uint32_t tile = blockIdx.x;
    const int p = entry_of(prefix, B.n_planes, tile);
    const QualityPlane& P = B.planes[p];
    const int h = P.h >> scale, w = P.w >> scale;
    const int oh = h - (kQWin - 1), ow = w - (kQWin - 1);  // window positions ("valid"); >= 1 for a plane that has tiles
    const int tiles_x = (ow + kQTile - 1) / kQTile, tiles_y = (oh + kQTile - 1) / kQTile;
    const int t = static_cast<int>(tile - prefix[p]);
    const int tx = t % tiles_x, ty = t / tiles_x;
    const int x0 = tx * kQTile, y0 = ty * kQTile;
    const int tid = threadIdx.x;
    const void* px = scale == 0 ? P.src : static_cast<const void*>(P.pool[0][scale - 1]);
    const void* py = scale == 0 ? P.dec : static_cast<const void*>(P.pool[1][scale - 1]);
    const int kind = scale == 0 ? P.wide : 2;

    // ---- stage 42 x 42 samples of both pictures (zeros outside: they only reach window positions that are masked below)
    for (int i = tid; i < kQStage * kQStage; i += kThreads) {
        const int r = i / kQStage, c = i - r * kQStage;
        const int gy = y0 + r, gx = x0 + c;
        float a = 0.f, b = 0.f;
        if (gy < h && gx < w) {
            const size_t at = static_cast<size_t>(gy) * w + gx;
            a = load_sample(px, kind, at);
            b = load_sample(py, kind, at);
        }
        sx[r * kSX + c] = a;
        sy[r * kSX + c] = b;
    }
    __syncthreads();

    // ---- the next scale's pictures: 2 x 2 sums of the staged samples.  A tile owns the 16 x 16 pooled pixels under its
    // 32 x 32 corner; the last tile of a row / column also owns what lies under its halo (at most 21), so the tiles cover
    // the whole (h / 2) x (w / 2) picture exactly once.  A trailing odd row or column is dropped.
    if (scale + 1 < kQScales) {
        const int ph = h >> 1, pw = w >> 1;
        const int pr_n = ty == tiles_y - 1 ? ph - y0 / 2 : kQTile / 2;
        const int pc_n = tx == tiles_x - 1 ? pw - x0 / 2 : kQTile / 2;
        float* ox = P.pool[0][scale];
        float* oy = P.pool[1][scale];
        for (int i = tid; i < pr_n * pc_n; i += kThreads) {
            const int r = i / pc_n, c = i - r * pc_n;
            const int at = 2 * r * kSX + 2 * c;
            const size_t to = static_cast<size_t>(y0 / 2 + r) * pw + (x0 / 2 + c);
            ox[to] = (sx[at] + sx[at + 1]) + (sx[at + kSX] + sx[at + kSX + 1]);  // integers below 2^24: exact
            oy[to] = (sy[at] + sy[at + 1]) + (sy[at + kSX] + sy[at + kSX + 1]);
        }
    }

    // ---- horizontal pass: an item is 8 adjacent positions of one staged row, for all five maps
    for (int it = tid; it < kQStage * (kQTile / 8); it += kThreads) {
        const int r = it % kQStage, c0 = (it / kQStage) * 8;
        double vx[8 + kQWin - 1], vy[8 + kQWin - 1];
#pragma unroll
        for (int k = 0; k < 8 + kQWin - 1; ++k) {
            vx[k] = static_cast<double>(sx[r * kSX + c0 + k]);
            vy[k] = static_cast<double>(sy[r * kSX + c0 + k]);
        }
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            double ax = 0., ay = 0., axx = 0., ayy = 0., axy = 0.;
#pragma unroll
            for (int k = 0; k < kQWin; ++k) {
                const double gx_ = B.g[k] * vx[o + k], gy_ = B.g[k] * vy[o + k];
                ax += gx_;
                ay += gy_;
                axx = fma(gx_, vx[o + k], axx);
                ayy = fma(gy_, vy[o + k], ayy);
                axy = fma(gx_, vy[o + k], axy);
            }
            const int at = r * kHS + c0 + o;
            hm[0][at] = ax; hm[1][at] = ay; hm[2][at] = axx; hm[3][at] = ayy; hm[4][at] = axy;
        }
    }
    __syncthreads();

    // ---- vertical pass: a thread owns 4 rows of one column; then cs and ssim per window position
    const int c = tid % kQTile, r0 = (tid / kQTile) * 4;
    double m[5][4];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        double v[4 + kQWin - 1];
#pragma unroll
        for (int k = 0; k < 4 + kQWin - 1; ++k) v[k] = hm[q][(r0 + k) * kHS + c];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            double a = 0.;
#pragma unroll
            for (int k = 0; k < kQWin; ++k) a = fma(B.g[k], v[o + k], a);
            m[q][o] = a;
        }
    }
    double norm = P.inv_maxv;
    for (int k = 0; k < scale; ++k) norm *= 0.25;  // the staged values are sums of 4^scale samples
    const double norm2 = norm * norm;
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    double cs_sum = 0., ssim_sum = 0.;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        if (y0 + r0 + o < oh && x0 + c < ow) {
            const double mx = m[0][o] * norm, my = m[1][o] * norm;
            const double sxx = m[2][o] * norm2 - mx * mx, syy = m[3][o] * norm2 - my * my, sxy = m[4][o] * norm2 - mx * my;
            const double cs = (2. * sxy + C2) / (sxx + syy + C2);
            cs_sum += cs;
            ssim_sum += (2. * mx * my + C1) / (mx * mx + my * my + C1) * cs;
        }
    }
    cs_sum = wave_sum_f64(cs_sum);
    ssim_sum = wave_sum_f64(ssim_sum);
    if ((tid & 63) == 0) { wave_part[0][tid >> 6] = cs_sum; wave_part[1][tid >> 6] = ssim_sum; }
    __syncthreads();
    if (tid == 0) {
        double* out = B.ms_part + (static_cast<size_t>(B.scale_first[scale]) + tile) * 2;
        out[0] = ((wave_part[0][0] + wave_part[0][1]) + wave_part[0][2]) + wave_part[0][3];
        out[1] = ((wave_part[1][0] + wave_part[1][1]) + wave_part[1][2]) + wave_part[1][3];
    }
}

// One wave per (plane, k): k = 0 adds the plane's squared-error partials, k = 1 + j the cs / ssim partials of scale j.
__global__ __launch_bounds__(64) void quality_final_kernel(QualityBatch B) {
    const int p = blockIdx.x / (1 + kQScales), k = blockIdx.x % (1 + kQScales);
    const int lane = threadIdx.x;
    if (k == 0) {
        uint64_t acc = 0;
        for (uint32_t i = B.sse_prefix[p] + lane; i < B.sse_prefix[p + 1]; i += 64) acc += B.sse_part[i];
        acc = wave_sum_u64(acc);
        if (lane == 0) B.out[p].sse = acc;
        return;
    }
    const int j = k - 1;
    const uint32_t* prefix = B.ms_prefix + static_cast<size_t>(j) * (B.n_planes + 1);
    double cs = 0., ss = 0.;
    for (uint32_t i = prefix[p] + lane; i < prefix[p + 1]; i += 64) {
        const double* part = B.ms_part + (static_cast<size_t>(B.scale_first[j]) + i) * 2;
        cs += part[0];
        ss += part[1];
    }
    cs = wave_sum_f64(cs);
    ss = wave_sum_f64(ss);
    if (lane == 0) { B.out[p].cs_sum[j] = cs; B.out[p].ssim_sum[j] = ss; }
}

}  // namespace

// Enqueues the scoring of a planned batch (ccd_quality_api.cpp builds the tables).  n_sse_tiles == 0: no squared error asked for.
hipError_t launch_quality(const QualityBatch& B, uint32_t n_sse_tiles, hipStream_t stream) {
    if (n_sse_tiles) hipLaunchKernelGGL(quality_sse_kernel, dim3(n_sse_tiles), dim3(kThreads), 0, stream, B);
    for (int j = 0; j < kQScales; ++j) {
        const uint32_t tiles = B.scale_first[j + 1] - B.scale_first[j];
        if (tiles) hipLaunchKernelGGL(quality_msssim_kernel, dim3(tiles), dim3(kThreads), 0, stream, B, j);
    }
    hipLaunchKernelGGL(quality_final_kernel, dim3(static_cast<uint32_t>(B.n_planes) * (1 + kQScales)), dim3(64), 0, stream, B);
    return hipGetLastError();
}

}  // namespace ccd
