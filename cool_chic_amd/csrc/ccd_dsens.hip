// ccd_dsens.hip - the integer kernels of the distortion deltas (gfx950; DESIGN.md 4.13, include/ccd.h ccd_dsens_*).
//
// The planes of a moved latent come from the float path that exists (given-latent slots of a decode batch); what runs here
// is what stands around a round of up to K such passes:
//   dsens_apply_kernel  writes the probed grid of every probe slot's private latent copy: the caller's grid, with v + move
//                       on the pass's lattice where that stays inside [-64, 63]; and a plain copy of the grid a slot probed
//                       in the round before.  A segment is one grid of one copy; a 64-lane workgroup writes kDsensChunk
//                       bytes of it and finds it in a prefix table of workgroups, as latent_ingest_kernel does: 16-byte
//                       units where source and destination are aligned alike, bytes at the ragged ends.  The moves are byte
//                       stores of the same wave behind the copy.
//   dsens_sse_kernel    phase 0: a workgroup (one wave) sums (p - src)^2 - (b - src)^2 over one band of one probe's box, all
//                       three planes, and leaves the int64 in a slab.  Boxes of a pass are congruent up to clipping, so every
//                       probe of a pass owns the same number of bands and a unit finds its pass by bisection of a prefix
//                       table, its probe and band by division: 11 x 11 boxes of the finest grid are one band each, a box
//                       that covers the picture a hundred.
//                       phase 1: a lane per probe adds its bands in band order and stores the entry, or INT64_MIN where the
//                       move leaves the alphabet.
//   dsens_dep_final_kernel  the dependent maps of a run: sentinels over the sums dsens_dep_kernel (ccd_inter.hip) left,
//                       and the count of flagged entries per grid - the one integer atomic add of this file.
// Every sum is an integer sum: any order gives the same bits.  No waits; plain vector stores.
#include <hip/hip_runtime.h>

#include "ccd_kernels.hpp"

namespace ccd {
namespace {
__device__ __forceinline__ bool in_alphabet(int v) { return v >= kAcLo && v < kAcLo + kAlphabet; }

__global__ __launch_bounds__(64) void dsens_apply_kernel(const DsensSeg* __restrict__ segs, const uint32_t* __restrict__ prefix, int n_segs) {
    const uint32_t blk = blockIdx.x;
    const int s = entry_of(prefix, n_segs, blk);
    const DsensSeg S = segs[s];
    const uint32_t lane = threadIdx.x;
    const uint32_t o0 = (blk - prefix[s]) * kDsensChunk;  // (< n: the prefix gives a segment ceil(n / kDsensChunk) workgroups)
    const uint32_t n = S.n - o0 < kDsensChunk ? S.n - o0 : kDsensChunk;
    const int8_t* src = S.src + o0;
    int8_t* dst = S.dst + o0;
    // [0, head) bytes, [head, head + body) 16-byte units, [head + body, n) bytes
    uint32_t head = n, body = 0;
    const uintptr_t sa = reinterpret_cast<uintptr_t>(src), da = reinterpret_cast<uintptr_t>(dst);
    if (((sa ^ da) & 15) == 0) {
        const uint32_t to_16 = static_cast<uint32_t>((16 - (sa & 15)) & 15);
        head = to_16 < n ? to_16 : n;
        body = (n - head) & ~15u;
    }
    for (uint32_t i = lane; i < head; i += 64) dst[i] = src[i];
    for (uint32_t i = head + lane * 16; i < head + body; i += 64 * 16) *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(src + i);
    for (uint32_t i = head + body + lane; i < n; i += 64) dst[i] = src[i];
    if (S.move == 0) return;
    __syncthreads();  // one wave: the moves below follow the copy in program order
    // the lattice points of this chunk: rows ya .. yb of the grid, of those the ones congruent to py
    const uint32_t w = static_cast<uint32_t>(S.w), st = static_cast<uint32_t>(S.stride);
    const uint32_t ya = o0 / w, yb = (o0 + n - 1) / w;
    const uint32_t ly0 = ya + (static_cast<uint32_t>(S.py) + st - ya % st) % st;
    if (ly0 > yb || static_cast<uint32_t>(S.px) >= w) return;
    const uint32_t n_rows = (yb - ly0) / st + 1, nx = (w - 1 - static_cast<uint32_t>(S.px)) / st + 1;
    for (uint32_t it = lane; it < n_rows * nx; it += 64) {
        const uint32_t r = it / nx, c = it - r * nx;
        const uint32_t at = (ly0 + r * st) * w + static_cast<uint32_t>(S.px) + c * st;
        if (at < o0 || at >= o0 + n) continue;
        const int v = S.src[at];
        if (in_alphabet(v) && in_alphabet(v + S.move)) S.dst[at] = static_cast<int8_t>(v + S.move);
    }
}

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(static_cast<long long>(v), off, 64);
    return v;
}

template <typename T>
__device__ __forceinline__ int64_t band_sum(const void* base, const void* probe, const void* src, int pw, int r0, int r1, int c0, int c1,
                                            int lane) {
    const T* b = static_cast<const T*>(base);
    const T* p = static_cast<const T*>(probe);
    const T* s = static_cast<const T*>(src);
    const uint32_t bw = static_cast<uint32_t>(c1 - c0 + 1), cnt = static_cast<uint32_t>(r1 - r0 + 1) * bw;
    int64_t acc = 0;
    for (uint32_t i = lane; i < cnt; i += 64) {
        const uint32_t r = i / bw, c = i - r * bw;
        const size_t at = static_cast<size_t>(r0 + static_cast<int>(r)) * pw + (c0 + static_cast<int>(c));
        const int64_t sv = s[at], dp = static_cast<int64_t>(p[at]) - sv, db = static_cast<int64_t>(b[at]) - sv;
        acc += dp * dp - db * db;
    }
    return acc;
}

__global__ __launch_bounds__(64) void dsens_sse_kernel(const DsensPass* __restrict__ passes, const uint32_t* __restrict__ unit_prefix,
                                                       const uint32_t* __restrict__ probe_prefix, int n_passes, int64_t* __restrict__ slab,
                                                       uint32_t n_probes, int phase) {
    const int lane = threadIdx.x;
    if (phase == 1) {
        const uint32_t q = blockIdx.x * 64u + lane;
        if (q >= n_probes) return;
        const int p = entry_of(probe_prefix, n_passes, q);
        const DsensPass& P = passes[p];
        const uint32_t lp = q - probe_prefix[p];
        const int iy = static_cast<int>(lp / static_cast<uint32_t>(P.nx)), ix = static_cast<int>(lp % static_cast<uint32_t>(P.nx));
        const int y = P.py + iy * P.stride, x = P.px + ix * P.stride;
        const size_t at = static_cast<size_t>(y) * P.w + x;
        const int v = P.lat[at];
        int64_t acc = 0;
        const int64_t* part = slab + unit_prefix[p] + static_cast<size_t>(lp) * P.upp;
        for (int t = 0; t < P.upp; ++t) acc += part[t];
        if (!in_alphabet(v + P.move)) acc = INT64_MIN;
        P.map[(P.move > 0 ? static_cast<size_t>(P.h) * P.w : 0) + at] = acc;
        return;
    }
    const uint32_t u = blockIdx.x;
    const int p = entry_of(unit_prefix, n_passes, u);
    const DsensPass& P = passes[p];
    const uint32_t lu = u - unit_prefix[p];
    int64_t acc = 0;
    if (!P.empty) {
        const uint32_t lp = lu / static_cast<uint32_t>(P.upp);
        const int band = static_cast<int>(lu % static_cast<uint32_t>(P.upp));
        const int iy = static_cast<int>(lp / static_cast<uint32_t>(P.nx)), ix = static_cast<int>(lp % static_cast<uint32_t>(P.nx));
        const int y = P.py + iy * P.stride, x = P.px + ix * P.stride;
        const int sy = static_cast<int>(static_cast<uint64_t>(y) * P.num_y / P.den_y), sx = static_cast<int>(static_cast<uint64_t>(x) * P.num_x / P.den_x);
        const int Y0 = max(sy + P.box[0], 0), Y1 = min(sy + P.box[2], P.H - 1);
        const int X0 = max(sx + P.box[1], 0), X1 = min(sx + P.box[3], P.W - 1);
        if (Y0 <= Y1 && X0 <= X1) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int sh = k ? P.chroma_shift : 0;
                const int ph = P.H >> sh, pw = P.W >> sh;  // 4:2:0 chroma: floor(H / 2) x floor(W / 2), 2 x 2 means of the full planes
                const int b0 = Y0 >> sh, b1 = min(Y1 >> sh, ph - 1), c0 = X0 >> sh, c1 = min(X1 >> sh, pw - 1);
                const int r0 = b0 + band * P.rows, r1 = min(r0 + P.rows - 1, b1);
                if (r0 > r1 || c0 > c1) continue;
                acc += P.wide ? band_sum<uint16_t>(P.base[k], P.probe[k], P.src[k], pw, r0, r1, c0, c1, lane)
                              : band_sum<uint8_t>(P.base[k], P.probe[k], P.src[k], pw, r0, r1, c0, c1, lane);
            }
        }
    }
    acc = wave_sum_i64(acc);
    if (lane == 0) slab[u] = acc;
}

// The dependent maps of a run, behind its last round: entry e of a grid's [2][h][w] is, in this order, INT64_MIN
// where the move leaves the alphabet, INT64_MIN where dsens_dep_kernel flagged a conflict, else the sum it accumulated.  A
// workgroup is 256 entries of one grid; the flagged legal entries are counted per grid (an integer sum: one atomic per wave).
__global__ __launch_bounds__(256) void dsens_dep_final_kernel(const DsensDepGrid* __restrict__ grids, const uint32_t* __restrict__ prefix, int n_grids) {
    const uint32_t blk = blockIdx.x;
    const int g = entry_of(prefix, n_grids, blk);
    const DsensDepGrid G = grids[g];
    const uint32_t e = (blk - prefix[g]) * 256u + threadIdx.x;
    bool counted = false;
    if (e < 2u * G.n) {
        const int v = G.lat[e < G.n ? e : e - G.n], move = e < G.n ? -1 : 1;
        const bool legal = in_alphabet(v + move), flagged = G.flag[e] != 0;
        if (!legal || flagged) G.map[e] = INT64_MIN;
        counted = legal && flagged;
    }
    const unsigned long long mask = __ballot(counted);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(G.conflicts, static_cast<unsigned long long>(__popcll(mask)));
}
}  // namespace

hipError_t launch_dsens_dep_final(const DsensDepGrid* d_grids, const uint32_t* d_prefix, int n_grids, uint32_t n_blocks, hipStream_t stream) {
    if (n_grids <= 0 || n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(dsens_dep_final_kernel, dim3(n_blocks), dim3(256), 0, stream, d_grids, d_prefix, n_grids);
    return hipGetLastError();
}

hipError_t launch_dsens_apply(const DsensSeg* d_segs, const uint32_t* d_prefix, int n_segs, uint32_t n_blocks, hipStream_t stream) {
    if (n_segs <= 0 || n_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(dsens_apply_kernel, dim3(n_blocks), dim3(64), 0, stream, d_segs, d_prefix, n_segs);
    return hipGetLastError();
}

hipError_t launch_dsens_sse(const DsensPass* d_passes, const uint32_t* d_unit_prefix, const uint32_t* d_probe_prefix, int n_passes,
                            uint32_t n_units, uint32_t n_probes, int64_t* d_slab, hipStream_t stream) {
    if (n_passes <= 0 || n_units == 0 || n_probes == 0) return hipSuccess;
    hipLaunchKernelGGL(dsens_sse_kernel, dim3(n_units), dim3(64), 0, stream, d_passes, d_unit_prefix, d_probe_prefix, n_passes, d_slab, n_probes, 0);
    hipLaunchKernelGGL(dsens_sse_kernel, dim3((n_probes + 63) / 64), dim3(64), 0, stream, d_passes, d_unit_prefix, d_probe_prefix, n_passes,
                       d_slab, n_probes, 1);
    return hipGetLastError();
}
}  // namespace ccd
