// ccd_rdoq.hip - one RDOQ step: choose and apply +-1 moves of latents that provably do not interact (gfx950, wave64;
// DESIGN.md 4.14, include/ccd.h ccd_rdoq_*).
//
// Inputs are the two delta maps of every grid (distortion: int64, rate: float32) and, per latent, its influence box in cells
// of the slot's claim raster (built on the host by the code behind ccd_rdoq_influence_box).  Two latents whose boxes share no
// cell neither share a symbol of the rate model nor a sample of the planes, so their deltas add.
//   rdoq_claim_kernel   the cost of both moves of a latent, its better move, whether that is a candidate, its 64-bit key
//                       (cost as an ordered float, then the latent's number); a candidate does atomicMin of the key into every
//                       cell of its box.  The smallest key wins a cell whatever the order of the atomics.
//   rdoq_select_kernel  a candidate that finds its own key in every cell of its box is selected: the latent is stored as v + s
//                       (a byte store into the caller's grid), the move map gets s, every other latent's entry 0.
//   rdoq_reduce_kernel  phase 0: a workgroup sums candidates, moves, dD and dBits of one chunk of one grid; phase 1: a wave
//                       per slot adds the chunks grid by grid, writes the result and stores all ones into the claim raster.
// Work is dealt out by cells: a workgroup is one wave, and it is either 64 latents of one grid, a lane each, for boxes of
// up to kRdoqLaneCells cells, or ONE latent with a larger box (the grid's `big` list), the lanes over its cells.  A workgroup
// finds its grid by bisection of a prefix table, as the dsens kernels do.
//
// The raster.  claim needs all ones.  select is the raster's last reader of a step; phase 1 of the reduce launch follows it on
// the stream and stores all ones with plain vector stores; the next step's claim follows that launch on the stream.  Each word
// is written by one kind of access per launch (atomics in claim, plain stores in reduce), and launches are ordered by their
// stream: no access of one launch meets one of another.  The first step finds the ones ccd_rdoq_add left.
//
// Sums: integers in any order; dBits in float64 in an order that is a function of the geometry alone (a lane adds its latents
// in ascending order, a fixed shuffle tree adds the lanes, chunks and grids are added in ascending order).  No float atomics.
#include <hip/hip_runtime.h>

#include "ccd_kernels.hpp"

namespace ccd {
namespace {
__device__ __forceinline__ bool in_alphabet(int v) { return v >= kAcLo && v < kAcLo + kAlphabet; }

// Floats in the order of their values as unsigned integers.
__device__ __forceinline__ uint32_t ordered(float c) {
    const uint32_t b = __float_as_uint(c);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

struct Move { int pick; int s; unsigned long long key; };  // pick: 0 no candidate, 1 / 2 candidate for -1 / +1

// Rule steps 1-3 for latent i of grid G.  Separate roundings of the two products and of the sum: what numpy float64 does.
__device__ __forceinline__ Move best_move(const RdoqGrid& G, const RdoqSlot& S, uint32_t i) {
    const int v = G.lat[i];
    double c64[2];
    bool exists[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int64_t dd = G.dd ? G.dd[static_cast<size_t>(k) * G.n + i] : 0;
        const float db = G.db[static_cast<size_t>(k) * G.n + i];
        exists[k] = in_alphabet(v) && in_alphabet(v + 2 * k - 1) && dd != INT64_MIN && isfinite(db);
        c64[k] = __dadd_rn(__dmul_rn(static_cast<double>(dd), S.kD), __dmul_rn(static_cast<double>(db), S.kR));
    }
    const float c32[2] = {static_cast<float>(c64[0]), static_cast<float>(c64[1])};
    const int k = exists[0] && exists[1] ? (c32[1] < c32[0] ? 1 : 0) : (exists[1] ? 1 : 0);
    Move m;
    m.s = 2 * k - 1;
    const bool admitted = G.grid < 64 && ((S.grid_mask >> G.grid) & 1);
    m.pick = (admitted && exists[k] && c64[k] < -S.min_gain) ? 1 + k : 0;
    m.key = (static_cast<unsigned long long>(ordered(c32[k])) << 32) | (G.first + i);
    return m;
}

// The box clipped to the raster once more: the table is the host's, the stores below are this kernel's.
struct Cells { uint32_t top, left, bh, bw, n; };
__device__ __forceinline__ Cells cells_of(const RdoqBox b, const RdoqSlot& S) {
    Cells c;
    const uint32_t bottom = min(static_cast<uint32_t>(b.bottom), static_cast<uint32_t>(S.cells_h - 1));
    const uint32_t right = min(static_cast<uint32_t>(b.right), static_cast<uint32_t>(S.cells_w - 1));
    c.top = min(static_cast<uint32_t>(b.top), bottom);
    c.left = min(static_cast<uint32_t>(b.left), right);
    c.bh = bottom - c.top + 1;
    c.bw = right - c.left + 1;
    c.n = c.bh * c.bw;
    return c;
}

// kSelect == false: claim.  kSelect == true: select and apply.
template <bool kSelect>
__device__ __forceinline__ void step_body(const RdoqGrid* __restrict__ grids, const RdoqSlot* __restrict__ slots,
                                          const uint32_t* __restrict__ lane_prefix, const uint32_t* __restrict__ big_prefix, int n_grids,
                                          uint32_t n_lane_blocks) {
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x < n_lane_blocks) {  // a lane per latent
        const int e = entry_of(lane_prefix, n_grids, blockIdx.x);
        const RdoqGrid& G = grids[e];
        const RdoqSlot& S = slots[G.slot];
        const uint32_t i = (blockIdx.x - lane_prefix[e]) * 64u + lane;
        if (i >= G.n) return;
        const Cells c = cells_of(G.box[i], S);
        if (c.n > kRdoqLaneCells) return;  // a wave's
        if (!kSelect) {
            const Move m = best_move(G, S, i);
            G.pick[i] = static_cast<uint8_t>(m.pick);
            if (m.pick)
                for (uint32_t r = 0; r < c.bh; ++r)
                    for (uint32_t q = 0; q < c.bw; ++q) atomicMin(&S.raster[static_cast<size_t>(c.top + r) * S.cells_w + c.left + q], m.key);
        } else {
            int s = 0;
            if (G.pick[i]) {
                const Move m = best_move(G, S, i);
                bool mine = true;
                for (uint32_t r = 0; r < c.bh; ++r)
                    for (uint32_t q = 0; q < c.bw; ++q) mine = mine && S.raster[static_cast<size_t>(c.top + r) * S.cells_w + c.left + q] == m.key;
                if (mine) {
                    s = m.s;
                    G.lat[i] = static_cast<int8_t>(G.lat[i] + s);
                }
            }
            G.moves[i] = static_cast<int8_t>(s);
        }
        return;
    }
    // one latent, the lanes over its cells
    const uint32_t u = blockIdx.x - n_lane_blocks;
    const int e = entry_of(big_prefix, n_grids, u);
    const RdoqGrid& G = grids[e];
    const RdoqSlot& S = slots[G.slot];
    const uint32_t i = G.big[u - big_prefix[e]];
    if (i >= G.n) return;
    const Cells c = cells_of(G.box[i], S);
    if (!kSelect) {
        const Move m = best_move(G, S, i);
        if (lane == 0) G.pick[i] = static_cast<uint8_t>(m.pick);
        if (m.pick)
            for (uint32_t t = lane; t < c.n; t += 64) {
                const uint32_t r = t / c.bw, q = t - r * c.bw;
                atomicMin(&S.raster[static_cast<size_t>(c.top + r) * S.cells_w + c.left + q], m.key);
            }
    } else {
        int s = 0;
        if (G.pick[i]) {  // (the same in every lane)
            const Move m = best_move(G, S, i);
            bool mine = true;
            for (uint32_t t = lane; t < c.n; t += 64) {
                const uint32_t r = t / c.bw, q = t - r * c.bw;
                mine = mine && S.raster[static_cast<size_t>(c.top + r) * S.cells_w + c.left + q] == m.key;
            }
            if (__all(mine)) s = m.s;
            // every lane has read the latent (best_move) before lane 0 stores it: one wave, program order
            if (lane == 0 && s) G.lat[i] = static_cast<int8_t>(G.lat[i] + s);
        }
        if (lane == 0) G.moves[i] = static_cast<int8_t>(s);
    }
}

__global__ __launch_bounds__(64) void rdoq_claim_kernel(const RdoqGrid* __restrict__ grids, const RdoqSlot* __restrict__ slots,
                                                        const uint32_t* __restrict__ lane_prefix, const uint32_t* __restrict__ big_prefix,
                                                        int n_grids, uint32_t n_lane_blocks) {
    step_body<false>(grids, slots, lane_prefix, big_prefix, n_grids, n_lane_blocks);
}

__global__ __launch_bounds__(64) void rdoq_select_kernel(const RdoqGrid* __restrict__ grids, const RdoqSlot* __restrict__ slots,
                                                         const uint32_t* __restrict__ lane_prefix, const uint32_t* __restrict__ big_prefix,
                                                         int n_grids, uint32_t n_lane_blocks) {
    step_body<true>(grids, slots, lane_prefix, big_prefix, n_grids, n_lane_blocks);
}

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(static_cast<long long>(v), off, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {  // a fixed tree: lane 0 holds ((l0 + l32) + (l16 + l48)) + ...
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = __dadd_rn(v, __shfl_down(v, off, 64));
    return v;
}

__global__ __launch_bounds__(64) void rdoq_reduce_kernel(const RdoqGrid* __restrict__ grids, const RdoqSlot* __restrict__ slots,
                                                         const uint32_t* __restrict__ chunk_prefix, int n_grids,
                                                         RdoqPartial* __restrict__ partial, ccd_rdoq_result* __restrict__ results, int phase) {
    const uint32_t lane = threadIdx.x;
    RdoqPartial acc = {0, 0, 0, 0.0};
    if (phase == 0) {
        const int e = entry_of(chunk_prefix, n_grids, blockIdx.x);
        const RdoqGrid& G = grids[e];
        const uint32_t i0 = (blockIdx.x - chunk_prefix[e]) * kRdoqChunk;
        const uint32_t i1 = min(i0 + kRdoqChunk, G.n);
        for (uint32_t i = i0 + lane; i < i1; i += 64) {
            acc.n_candidates += G.pick[i] != 0;
            const int s = G.moves[i];
            if (s == 0) continue;
            const size_t at = (s > 0 ? static_cast<size_t>(G.n) : 0) + i;
            acc.n_moves += 1;
            acc.d_sse += G.dd ? G.dd[at] : 0;
            acc.d_bits = __dadd_rn(acc.d_bits, static_cast<double>(G.db[at]));
        }
    } else {
        const RdoqSlot& S = slots[blockIdx.x];
        ccd_rdoq_result& R = results[blockIdx.x];
        RdoqPartial total = {0, 0, 0, 0.0};
        for (int g = 0; g < S.n_grids; ++g) {
            const int e = S.first_grid + g;
            acc = {0, 0, 0, 0.0};
            for (uint32_t c = chunk_prefix[e] + lane; c < chunk_prefix[e + 1]; c += 64) {
                const RdoqPartial P = partial[c];
                acc.n_candidates += P.n_candidates;
                acc.n_moves += P.n_moves;
                acc.d_sse += P.d_sse;
                acc.d_bits = __dadd_rn(acc.d_bits, P.d_bits);
            }
            acc.n_candidates = wave_sum_i64(acc.n_candidates);
            acc.n_moves = wave_sum_i64(acc.n_moves);
            acc.d_sse = wave_sum_i64(acc.d_sse);
            acc.d_bits = wave_sum_f64(acc.d_bits);
            if (lane == 0) R.n_moves_grid[g] = acc.n_moves;
            total.n_candidates += acc.n_candidates;
            total.n_moves += acc.n_moves;
            total.d_sse += acc.d_sse;
            total.d_bits = __dadd_rn(total.d_bits, acc.d_bits);
        }
        for (int g = S.n_grids + static_cast<int>(lane); g < CCD_MAX_GRIDS; g += 64) R.n_moves_grid[g] = 0;  // the block is the pool's
        if (lane == 0) {
            R.status = CCD_OK;
            R.n_grids = S.n_grids;
            R.n_candidates = total.n_candidates;
            R.n_moves = total.n_moves;
            R.d_sse = total.d_sse;
            R.d_bits = total.d_bits;
            R.d_cost = 0.0;  // the host's
        }
        // all ones for the next step's claim (the ordering argument is at the head of this file)
        uint4* words = reinterpret_cast<uint4*>(S.raster);
        for (uint32_t t = lane; t < S.raster_units; t += 64) words[t] = make_uint4(~0u, ~0u, ~0u, ~0u);
        return;
    }
    acc.n_candidates = wave_sum_i64(acc.n_candidates);
    acc.n_moves = wave_sum_i64(acc.n_moves);
    acc.d_sse = wave_sum_i64(acc.d_sse);
    acc.d_bits = wave_sum_f64(acc.d_bits);
    if (lane == 0) partial[blockIdx.x] = acc;
}
}  // namespace

hipError_t launch_rdoq_step(const RdoqGrid* d_grids, const RdoqSlot* d_slots, const uint32_t* d_lane_prefix, const uint32_t* d_big_prefix,
                            const uint32_t* d_chunk_prefix, int n_grids, int n_slots, uint32_t n_lane_blocks, uint32_t n_big,
                            uint32_t n_chunks, RdoqPartial* d_partial, ccd_rdoq_result* d_results, hipStream_t stream) {
    if (n_grids <= 0 || n_slots <= 0 || n_lane_blocks == 0 || n_chunks == 0) return hipSuccess;
    const dim3 units(n_lane_blocks + n_big);
    hipLaunchKernelGGL(rdoq_claim_kernel, units, dim3(64), 0, stream, d_grids, d_slots, d_lane_prefix, d_big_prefix, n_grids, n_lane_blocks);
    hipLaunchKernelGGL(rdoq_select_kernel, units, dim3(64), 0, stream, d_grids, d_slots, d_lane_prefix, d_big_prefix, n_grids, n_lane_blocks);
    hipLaunchKernelGGL(rdoq_reduce_kernel, dim3(n_chunks), dim3(64), 0, stream, d_grids, d_slots, d_chunk_prefix, n_grids, d_partial, d_results, 0);
    hipLaunchKernelGGL(rdoq_reduce_kernel, dim3(n_slots), dim3(64), 0, stream, d_grids, d_slots, d_chunk_prefix, n_grids, d_partial, d_results, 1);
    return hipGetLastError();
}
}  // namespace ccd
