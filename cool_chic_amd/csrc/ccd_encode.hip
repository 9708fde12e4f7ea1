// ccd_encode.hip - the WRITER on the device: range-encodes the latent grids of a cool-chic into exactly the bytes the
// host writer (ccd_writer.cpp, ccd_encode_coolchic) produces.  DESIGN.md section 4.10.
//
// Reference behaviour restated here (paths relative to /root/reference/coolchic):
//   bitstream/component/latent.py:142-173    the encoder walks the decoder's integer path in coding order (ccd_wavefront.hpp)
//   bitstream/component/coolchic.py:94-146   IFCE features on the nearest-upsampled stack of the coarser grids
//   bitstream/component/armint.py:180-203    fixed-point MLP (int64, wrap-around)
//   bitstream/component/rangecoder.py:46-76  -> constriction 0.4.2 RangeEncoder + QuantizedLaplace(-64,63)
//
// The decoder is serial because a pixel's context is made of symbols it has to decode first.  The encoder knows every
// latent up front, so only the coder's interval recurrence is serial.  Two kernels:
//   1. encode_contexts_kernel: one work item per latent pixel of every grid of every slot.  Gathers the causal
//      neighbours, evaluates the IFCE features of its position, runs the ARM in plain wrapping 64-bit arithmetic and
//      writes the pixel's interval (left, right - left) at the pixel's position IN CODING ORDER.
//   2. encode_chain_kernel: one wave per slot walks those intervals and runs the range encoder.  The intervals are
//      fetched 64 at a time by the whole wave; the recurrence is wave-uniform and runs on the scalar unit; words leave
//      through ordinary vector stores of lane 0.
// The rate meter (encode_rate_kernel, encode_rate_final_kernel) shares stage 1's per-pixel work and sums 24 - log2(width)
// per grid instead of running the chain.
#include <hip/hip_runtime.h>

#include "ccd_device.hpp"
#include "ccd_kernels.hpp"
#include "ccd_laplace.hpp"
#include "ccd_wavefront.hpp"

namespace ccd {

constexpr int kEncThreads = 64;  // one wave per workgroup: a lane only ever reads the LDS column it wrote (no barrier)

// ---- what every stage-1 kernel does for one pixel ---------------------------------------------------------------
// The Laplace parameters (mu, 1 / scale) of the pixel (y, x) of grid g: neighbour gather, IFCE features of (y >> 1, x >> 1),
// the wrapping 64-bit ARM, the clamp to table indices.  g is wave-uniform, so every weight is a scalar load; `smem_raw` holds
// the activations as [k][lane] columns and a lane only touches its own column.  No cross-lane operation in here: a caller
// may skip it for some lanes.
// kOverride: the one latent `ov` names is taken as ov.val wherever the pixel reads it (a spatial tap when ov.grid == g, an
// IFCE source when ov.grid > g), memory stays as it is - the delta kernels' "what if".  Without it `ov` is not looked at and
// the function is what it was before it had the parameter.
// kMove: whose entry `mv` moves - the parameter tables' "what if"; kRateDeltaNone: `mv` is not looked at.
//   kRateDeltaArm: one entry of the fixed-point ARM is taken as entry + mv.inc.  The sums are wrapping 64-bit, a
//   ring, so the unit's accumulator with that entry is the accumulator as it is plus mv.inc times the unit's input mv.in (times
//   one for a bias), bit for bit; mv is wave-uniform and the weights stay scalar loads.
//   kRateDeltaIfce: one entry of the fixed-point IFCE of grid mv.at is taken as entry + mv.inc (ifce_feature).
// kInputsOnly: the ARM's inputs (contexts and IFCE features) are left in the first dim columns and nothing else is done - the
// incremental path of the parameter tables keeps them there.
struct LatentOverride { int grid, y, x, val; };
// table indices (latent.py:156-165, rangecoder.py:90-91) of the ARM's two sums, as the Laplace parameters
__device__ __forceinline__ void arm_sums_to_model(const EntropyParams& P, uint64_t st0, uint64_t st1, double& mu, double& rcp) {
    const int64_t mi = (static_cast<int64_t>(st0) >> 24) + kMuOffset, si = (static_cast<int64_t>(st1) >> 24) + kScaleOffset;
    const int mu_idx = static_cast<int>(mi < 0 ? 0 : (mi > kNumMu - 1 ? kNumMu - 1 : mi));
    const int sc_idx = static_cast<int>(si < 0 ? 0 : (si > kNumScale - 1 ? kNumScale - 1 : si));

    mu = -64.0 + static_cast<double>(mu_idx) * (1.0 / 256.0);
    rcp = P.rcp_table[sc_idx];
}
// Feature o of the position (fy, fx) of grid g (coolchic.py:94-146): the accumulate over the fin source channels, the >> 24 and
// the .to(torch.float) / back to int64 round trip around F.interpolate (coolchic.py:142-144).  fw_ / fb_: the grid's w[fin][n_if]
// and b[n_if]; first: the stack is a single all-zero channel (coolchic.py:95-96).  kCand: the entry im names is taken as
// entry + im.inc (the IFCE table's "what if"): the accumulator is a ring, so it is the accumulator as it is plus
// im.inc times the source (times one for a bias); the caller has checked im.at == g and im.out == o.  The base and the
// candidate of either path of the table go through this one function.
template <bool kOverride, bool kCand>
__device__ __forceinline__ int64_t ifce_feature(const EntropyParams& P, int g, int fy, int fx, int o, int n_if, int fin, bool first,
                                                int base_level, const int64_t* fw_, const int64_t* fb_, const LatentOverride& ov,
                                                const RateDeltaMove& im) {
    uint64_t acc = static_cast<uint64_t>(fb_[o]);
    if (kCand && im.in < 0) acc += static_cast<uint64_t>(im.inc);
    if (!first) {
        for (int c = 0; c < fin; ++c) {
            const int m = g + 1 + c;
            const int sh = P.level[m] - base_level;
            int64_t v = P.latent[m][(fy >> sh) * P.grid_w[m] + (fx >> sh)];
            if (kOverride && m == ov.grid && (fy >> sh) == ov.y && (fx >> sh) == ov.x) v = ov.val;
            acc += static_cast<uint64_t>(v << 16) * static_cast<uint64_t>(fw_[c * n_if + o]);
            if (kCand && c == im.in) acc += static_cast<uint64_t>(v << 16) * static_cast<uint64_t>(im.inc);
        }
    }
    const int64_t q8 = static_cast<int64_t>(acc) >> 24;
    return static_cast<int32_t>(static_cast<int64_t>(static_cast<float>(q8)));
}
template <bool kOverride, int kMove = kRateDeltaNone, bool kInputsOnly = false>
__device__ __forceinline__ void encode_pixel_model(const EntropyParams& P, int g, int y, int x, int lane, unsigned char* smem_raw,
                                                   const LatentOverride& ov, double& mu, double& rcp, const RateDeltaMove& mv = RateDeltaMove{}) {
    const int dim = P.dim, n_sp = P.n_spatial, n_if = P.has_ifce ? P.n_ifce_out : 0;
    int64_t* xa = reinterpret_cast<int64_t*>(smem_raw) + lane;  // [dim][64], this lane's column
    int64_t* xb = xa + dim * kEncThreads;                       // [dim][64]
    const int8_t* __restrict__ lat = P.latent[g];
    const int n_grids = P.n_grids, W = P.grid_w[g];

    // ---- contexts, already << 16 (armint.py:193) ----
    for (int k = 0; k < n_sp; ++k) {
        const int yy = y - P.ctx_dy[k], xx = x + P.ctx_dx[k];
        int64_t v = (yy >= 0 && xx >= 0 && xx < W) ? lat[yy * W + xx] : 0;
        if (kOverride && g == ov.grid && yy == ov.y && xx == ov.x) v = ov.val;
        xa[k * kEncThreads] = static_cast<int64_t>(static_cast<uint64_t>(v) << 16);
    }
    // IFCE features of (y >> 1, x >> 1) at the coarser neighbour's size (coolchic.py:94-146).  Evaluated here, per
    // pixel, instead of once per feature position: four pixels share a position, so the work is done four times, but
    // it is ~5 % of the ARM's and no feature plane and no second pass exist.
    const int fin = P.ifce_in[g];
    if (fin > 0) {
        const int64_t* fw_ = P.ifce + P.ifce_off[g];  // w[fin][n_if]
        const int64_t* fb_ = fw_ + fin * n_if;
        const int fy = y >> 1, fx = x >> 1;
        const bool first = g == n_grids - 1;          // the stack is a single all-zero channel (coolchic.py:95-96)
        const int base_level = first ? 0 : P.level[g + 1];
        for (int o = 0; o < n_if; ++o) {
            int64_t f;
            if (kMove == kRateDeltaIfce && mv.at == g && mv.out == o) f = ifce_feature<kOverride, true>(P, g, fy, fx, o, n_if, fin, first, base_level, fw_, fb_, ov, mv);
            else f = ifce_feature<kOverride, false>(P, g, fy, fx, o, n_if, fin, first, base_level, fw_, fb_, ov, mv);
            xa[(n_sp + o) * kEncThreads] = static_cast<int64_t>(static_cast<uint64_t>(f) << 16);
        }
    } else {
        for (int o = 0; o < n_if; ++o) xa[(n_sp + o) * kEncThreads] = 0;
    }
    if (kInputsOnly) return;

    // ---- ARM (armint.py:180-203): stabiliser branch, hidden layers, output layer; weights are wave-uniform reads ----
    const int64_t* ws = P.arm + (P.arm_len - 2 - 2 * dim);
    const int64_t* bs = ws + 2 * dim;
    uint64_t st0 = static_cast<uint64_t>(bs[0]), st1 = static_cast<uint64_t>(bs[1]);
    for (int k = 0; k < dim; ++k) {
        const uint64_t v = static_cast<uint64_t>(xa[k * kEncThreads]);
        st0 += v * static_cast<uint64_t>(ws[k * 2]);
        st1 += v * static_cast<uint64_t>(ws[k * 2 + 1]);
    }
    if (kMove == kRateDeltaArm && mv.at == P.n_layers) {
        const uint64_t c = static_cast<uint64_t>(mv.inc) * (mv.in < 0 ? uint64_t{1} : static_cast<uint64_t>(xa[mv.in * kEncThreads]));
        if (mv.out == 0) st0 += c; else st1 += c;
    }
    int64_t* xin = xa;
    int64_t* xout = xb;
    const int64_t* lw = P.arm;
    for (int l = 0; l < P.n_layers - 1; ++l) {
        const int64_t* lb = lw + dim * dim;
        for (int o = 0; o < dim; o += 2) {  // two outputs per pass: two independent accumulator chains
            const int o1 = min(o + 1, dim - 1);
            uint64_t a0 = static_cast<uint64_t>(lb[o]), a1 = static_cast<uint64_t>(lb[o1]);
#pragma unroll 2
            for (int k = 0; k < dim; ++k) {
                const uint64_t v = static_cast<uint64_t>(xin[k * kEncThreads]);
                a0 += v * static_cast<uint64_t>(lw[k * dim + o]);
                a1 += v * static_cast<uint64_t>(lw[k * dim + o1]);
            }
            if (kMove == kRateDeltaArm && mv.at == l && (mv.out == o || mv.out == o1)) {
                const uint64_t c = static_cast<uint64_t>(mv.inc) * (mv.in < 0 ? uint64_t{1} : static_cast<uint64_t>(xin[mv.in * kEncThreads]));
                if (mv.out == o) a0 += c;
                if (mv.out == o1) a1 += c;
            }
            const int64_t v0 = static_cast<int64_t>(a0), v1 = static_cast<int64_t>(a1);
            xout[o * kEncThreads] = (v0 < 0 ? 0 : v0) >> 16;
            xout[o1 * kEncThreads] = (v1 < 0 ? 0 : v1) >> 16;
        }
        int64_t* t = xin; xin = xout; xout = t;
        lw = lb + dim;
    }
    {
        const int64_t* lb = lw + dim * 2;
        uint64_t a0 = static_cast<uint64_t>(lb[0]), a1 = static_cast<uint64_t>(lb[1]);
        for (int k = 0; k < dim; ++k) {
            const uint64_t v = static_cast<uint64_t>(xin[k * kEncThreads]);
            a0 += v * static_cast<uint64_t>(lw[k * 2]);
            a1 += v * static_cast<uint64_t>(lw[k * 2 + 1]);
        }
        if (kMove == kRateDeltaArm && mv.at == P.n_layers - 1) {
            const uint64_t c = static_cast<uint64_t>(mv.inc) * (mv.in < 0 ? uint64_t{1} : static_cast<uint64_t>(xin[mv.in * kEncThreads]));
            if (mv.out == 0) a0 += c; else a1 += c;
        }
        st0 += a0; st1 += a1;
    }
    arm_sums_to_model(P, st0, st1, mu, rcp);
}

// The interval [left, right) of symbol `sym` (already checked to be in the alphabet) at (y, x) of grid g under the leaky
// quantised Laplace model: window_left of sym and sym + 1.
__device__ __forceinline__ void encode_pixel_interval(const EntropyParams& P, int g, int y, int x, int sym, int lane,
                                                      unsigned char* smem_raw, uint32_t& left, uint32_t& right) {
    double mu, rcp;
    encode_pixel_model<false>(P, g, y, x, lane, smem_raw, LatentOverride{}, mu, rcp);
    left = window_left(mu, rcp, sym, kExpTab);           // 0 for -64
    right = window_left(mu, rcp, sym + 1, kExpTab);      // 2^24 for 63
}

// ---- stage 1: contexts ------------------------------------------------------------------------------------------
// blockIdx.y = slot, blockIdx.x = index into the slot's blocks: every grid owns ceil(H * W / 64) consecutive blocks
// (EncodeParams::block_first), so the grid - and with it every network offset - is uniform in a workgroup.
__global__ __launch_bounds__(kEncThreads) void encode_contexts_kernel(const EncodeParams* slots) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const EncodeParams& Q = slots[blockIdx.y];
    const EntropyParams& P = Q.ep;
    if (blockIdx.x >= Q.n_blocks) return;
    const int lane = threadIdx.x;
    const int n_grids = P.n_grids;
    int g = 0;
    while (g + 1 < n_grids && blockIdx.x >= Q.block_first[g + 1]) ++g;  // block_first grows with g
    const int H = P.grid_h[g], W = P.grid_w[g];
    const int p = static_cast<int>(blockIdx.x - Q.block_first[g]) * kEncThreads + lane;
    if (p >= H * W) return;
    const int y = p / W, x = p - y * W;

    // the pixel's own symbol: checked before anything depends on it (the host writer: CCD_ERR_VALUE)
    const int sym = P.latent[g][p];
    if (sym < kAcLo || sym > kAcLo + kAlphabet - 1) { P.status[0] = CCD_ERR_VALUE; return; }
    uint32_t left, right;
    encode_pixel_interval(P, g, y, x, sym, lane, smem_raw, left, right);

    // ---- position in coding order (ccd_wavefront.hpp): the pixels in front of its step, then the rows of the step above it ----
    uint32_t idx = Q.grid_first[g];
    if (wf_raster(W)) idx += static_cast<uint32_t>(p);
    else {
        const int c = wf_step_of(y, x);
        const int y0 = wf_first_row(W, c);
        idx += Q.step_prefix[g][c] + static_cast<uint32_t>(y - y0);
    }
    Q.pairs[idx] = EncodePair{left, right - left};
}

// ---- stage 2: the interval chain --------------------------------------------------------------------------------
// constriction's RangeEncoder as ccd_writer.cpp:41-83 restates it, one wave per slot.  Every value of the recurrence
// is the same in all lanes (it is made of v_readlane results and constants), so the compiler keeps it in scalar
// registers; the only vector work is the fetch of the next 64 intervals and the stores of lane 0.
// status: [0] error, [1] words written, [2] times an "inverted" run began, [3] runs resolved WITH a carry,
//         [4] runs resolved without one (the carry path is exercised, not assumed).
__global__ __launch_bounds__(kEncThreads) void encode_chain_kernel(const EncodeParams* slots) {
    const EncodeParams& Q = slots[blockIdx.x];
    int32_t* status = Q.ep.status;
    const int lane = threadIdx.x;
    if (status[0] != 0) return;  // a symbol outside the alphabet: the slot emits nothing
    const uint32_t n = Q.n_symbols, cap = Q.cap_words;
    uint32_t* __restrict__ out = Q.out;
    const EncodePair* __restrict__ pairs = Q.pairs;

    uint64_t lower = 0, range = ~uint64_t{0};
    bool inverted = false;
    uint32_t n_inverted = 0, first_inverted = 0, pos = 0;
    uint32_t n_runs = 0, n_carry = 0, n_plain = 0;
    auto put_word = [&](uint32_t w) {
        if (lane == 0 && pos < cap) out[pos] = w;
        ++pos;
    };
    auto flush_inverted = [&](bool carry) {
        put_word(carry ? first_inverted + 1u : first_inverted);
        const uint32_t fill = carry ? 0u : 0xFFFFFFFFu, m = n_inverted - 1;
        for (uint32_t j = lane; j < m; j += kEncThreads) if (pos + j < cap) out[pos + j] = fill;
        pos += m;
        if (carry) ++n_carry; else ++n_plain;
    };

    EncodePair nxt{0u, 0u};
    if (static_cast<uint32_t>(lane) < n) nxt = pairs[lane];
    for (uint32_t base = 0; base < n; base += kEncThreads) {
        const EncodePair cur = nxt;
        const uint32_t ahead = base + kEncThreads + lane;
        if (ahead < n) nxt = pairs[ahead];  // in flight while this chunk's 64 symbols are coded
        const int cnt = static_cast<int>(min(static_cast<uint32_t>(kEncThreads), n - base));
        for (int i = 0; i < cnt; ++i) {
            const uint32_t l = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cur.left), i));
            const uint32_t w = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cur.width), i));
            const uint64_t scale = range >> kRcPrecision;
            range = scale * static_cast<uint64_t>(w);
            const uint64_t moved = lower + scale * l;
            if (inverted && static_cast<uint64_t>(moved + range) > moved) { flush_inverted(moved < lower); inverted = false; }
            lower = moved;
            if ((range >> 32) == 0) {
                const uint32_t word = static_cast<uint32_t>(lower >> 32);
                lower <<= 32; range <<= 32;
                if (inverted) ++n_inverted;
                else if (static_cast<uint64_t>(lower + range) > lower) put_word(word);
                else { inverted = true; n_inverted = 1; first_inverted = word; ++n_runs; }
            }
        }
    }
    if (n > 0) {  // seal
        const uint64_t point = lower + ((uint64_t{1} << 32) - 1);
        if (inverted) flush_inverted(point < lower);
        const uint32_t point_word = static_cast<uint32_t>(point >> 32);
        put_word(point_word);
        if (static_cast<uint32_t>(static_cast<uint64_t>(lower + range) >> 32) == point_word) put_word(0u);
    }
    if (lane == 0) {
        status[0] = pos <= cap ? 0 : CCD_ERR_NOMEM;  // (cannot happen: cap is ccd_enc_payload_bound)
        status[1] = static_cast<int32_t>(pos);
        status[2] = static_cast<int32_t>(n_runs);
        status[3] = static_cast<int32_t>(n_carry);
        status[4] = static_cast<int32_t>(n_plain);
    }
}

// ---- the rate meter: what the latents cost under the ARM, without the chain -----------------------------------------
// A symbol whose interval has width w out of 2^24 costs 24 - log2(w) bits; the chain only turns the intervals into bytes.
// Sums are formed in an order that depends on nothing but the grid's own size: 64 lanes through wave_sum's fixed tree, the
// workgroups' partials lane-strided in block order and through the same tree.  No atomics, so a slot gives the same 64 bits
// alone and inside any batch.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kEncThreads);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(v), off, kEncThreads));
    return v;
}

// Same grid as encode_contexts_kernel.  Tail lanes and lanes with a symbol outside the alphabet contribute 0 but stay
// for the reduction: no lane leaves before the shuffles (the early return below is for a whole workgroup).
__global__ __launch_bounds__(kEncThreads) void encode_rate_kernel(const EncodeParams* slots, const RateParams* rate) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const EncodeParams& Q = slots[blockIdx.y];
    const EntropyParams& P = Q.ep;
    const RateParams& R = rate[blockIdx.y];
    if (blockIdx.x >= Q.n_blocks) return;
    const int lane = threadIdx.x;
    const int n_grids = P.n_grids;
    int g = 0;
    while (g + 1 < n_grids && blockIdx.x >= Q.block_first[g + 1]) ++g;
    const int H = P.grid_h[g], W = P.grid_w[g];
    const int p = static_cast<int>(blockIdx.x - Q.block_first[g]) * kEncThreads + lane;
    double bits = 0.0;
    uint64_t width = 0;
    if (p < H * W) {
        const int sym = P.latent[g][p];
        if (sym < kAcLo || sym > kAcLo + kAlphabet - 1) R.status[0] = CCD_ERR_VALUE;
        else {
            const int y = p / W, x = p - y * W;
            uint32_t left, right;
            encode_pixel_interval(P, g, y, x, sym, lane, smem_raw, left, right);
            width = right - left;  // 1 .. 2^24
            bits = 24.0 - log2(static_cast<double>(width));
            if (R.map[g]) R.map[g][p] = static_cast<float>(bits);
        }
    }
    const double block_bits = wave_sum(bits);
    const uint64_t block_width = wave_sum(width);
    if (lane == 0) R.partial[blockIdx.x] = RatePartial{block_bits, block_width};
}

// One wave per (slot, grid): blockIdx.x = grid, blockIdx.y = slot.  Grid 0's wave also adds the per-grid sums up to the
// slot's total, so it walks every grid's partials itself (a total that waited for the other waves would need a second
// launch or a spin); the per-grid value it forms is the one that grid's own wave writes, addition for addition.
__device__ __forceinline__ RatePartial rate_grid_sum(const RatePartial* __restrict__ partial, uint32_t first, uint32_t last, int lane) {
    double bits = 0.0;
    uint64_t width = 0;
    for (uint32_t b = first + lane; b < last; b += kEncThreads) { bits += partial[b].bits; width += partial[b].sum_width; }
    return RatePartial{wave_sum(bits), wave_sum(width)};
}
__global__ __launch_bounds__(kEncThreads) void encode_rate_final_kernel(const EncodeParams* slots, const RateParams* rate) {
    const EncodeParams& Q = slots[blockIdx.y];
    const RateParams& R = rate[blockIdx.y];
    const int n_grids = Q.ep.n_grids, lane = threadIdx.x, g = blockIdx.x;
    if (g >= n_grids) return;
    const uint32_t last = g + 1 < n_grids ? Q.block_first[g + 1] : Q.n_blocks;
    const RatePartial s = rate_grid_sum(R.partial, Q.block_first[g], last, lane);
    if (lane == 0) R.grids[g] = RateGrid{s.bits, s.sum_width, static_cast<int64_t>(Q.ep.grid_h[g]) * Q.ep.grid_w[g]};
    if (g != 0) return;
    double total = s.bits;
    for (int m = 1; m < n_grids; ++m) {  // bounded by CCD_MAX_GRIDS
        const uint32_t end = m + 1 < n_grids ? Q.block_first[m + 1] : Q.n_blocks;
        total += rate_grid_sum(R.partial, Q.block_first[m], end, lane).bits;
    }
    if (lane == 0) *reinterpret_cast<double*>(R.grids + n_grids) = total;
}

// ---- rate sensitivity: what the slot's model bits would change by if ONE latent were v - 1 or v + 1 ---------------------
// DESIGN.md 4.10 "Rate sensitivity".  A latent p is read by its own symbol's model, by the pixels of its grid that hold it in a
// spatial tap, and by the pixels of finer grids whose IFCE feature reads it; each of them has p in exactly one context entry.
// Two launches behind the meter's, no atomics:
//   1. encode_delta_ifce_kernel: one wave per 8 x 8 tile of a fine grid, a lane per fine pixel.  For each of the pixel's
//      ifce_in sources the lane prices its own symbol with the source at v - 1 and v + 1 (the whole feature is recomputed,
//      float round trip included) against the price as it is; a fixed shuffle tree adds the lanes that share a source (or the
//      whole tile when the source's block is larger) and one lane stores the cell.
//   2. encode_delta_kernel: the grid of the contexts kernel, a lane per latent.  Own term from window_left at v - 1 .. v + 2
//      under the pixel's own (mu, rcp); then the spatial dependents in tap order, three model evaluations each; then the IFCE
//      cells of its block, fine grids in ascending order, cells in raster order.  float64 all the way, one float32 store.
__device__ __forceinline__ double log2_width(double mu, double rcp, int sym) {
    return log2(static_cast<double>(window_left(mu, rcp, sym + 1, kExpTab) - window_left(mu, rcp, sym, kExpTab)));
}
__device__ __forceinline__ bool in_alphabet(int sym) { return sym >= kAcLo && sym <= kAcLo + kAlphabet - 1; }

__global__ __launch_bounds__(kEncThreads) void encode_delta_ifce_kernel(const EncodeParams* slots, const DeltaParams* delta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const EntropyParams& P = slots[blockIdx.y].ep;
    const DeltaParams& D = delta[blockIdx.y];
    if (blockIdx.x >= D.n_tiles) return;
    const int lane = threadIdx.x;
    const int n_grids = P.n_grids;
    int g = 0;
    while (g + 1 < n_grids && blockIdx.x >= D.tile_first[g + 1]) ++g;  // tile_first grows with g; a grid without tiles owns none
    const int H = P.grid_h[g], W = P.grid_w[g];
    const int tiles_x = (W + kDeltaTile - 1) >> kDeltaTileLog;
    const int t = static_cast<int>(blockIdx.x - D.tile_first[g]);
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int qy = ty * kDeltaTile + (lane >> kDeltaTileLog), qx = tx * kDeltaTile + (lane & (kDeltaTile - 1));  // lane = y2 y1 y0 x2 x1 x0
    const bool inside = qy < H && qx < W;
    const int sym = inside ? P.latent[g][qy * W + qx] : 0;
    const bool ok = inside && in_alphabet(sym);  // the others hold 0 and stay for the shuffles
    double mu, rcp, base = 0.0;
    if (ok) {
        encode_pixel_model<false>(P, g, qy, qx, lane, smem_raw, LatentOverride{}, mu, rcp);
        base = log2_width(mu, rcp, sym);
    }
    const int fin = P.ifce_in[g], base_level = P.level[g + 1];
    double* cell = D.partial + D.part_first[g];
#pragma unroll 1
    for (int c = 0; c < fin; ++c) {
        const int m = g + 1 + c, sh = P.level[m] - base_level, s = delta_cell_shift(sh);
        double dm = 0.0, dp = 0.0;  // bits(q | source - 1) - bits(q), bits(q | source + 1) - bits(q)
        if (ok) {
            LatentOverride ov{m, (qy >> 1) >> sh, (qx >> 1) >> sh, 0};
            const int v = P.latent[m][ov.y * P.grid_w[m] + ov.x];
#pragma unroll 1
            for (int sign = -1; sign <= 1; sign += 2) {
                ov.val = v + sign;
                if (!in_alphabet(ov.val)) continue;  // the move does not exist: encode_delta_kernel stores +inf there
                encode_pixel_model<true>(P, g, qy, qx, lane, smem_raw, ov, mu, rcp);
                const double d = base - log2_width(mu, rcp, sym);
                if (sign < 0) dm = d; else dp = d;
            }
        }
        for (int j = 0; j < s; ++j) {  // s is wave-uniform: x0, y0, x1, y1, ..
            dm += __shfl_xor(dm, 1 << j, kEncThreads);
            dp += __shfl_xor(dp, 1 << j, kEncThreads);
            dm += __shfl_xor(dm, kDeltaTile << j, kEncThreads);
            dp += __shfl_xor(dp, kDeltaTile << j, kEncThreads);
        }
        const uint32_t n_cells = delta_cells(H, W, s);
        const int low = (1 << s) - 1;
        if (inside && (qy & low) == 0 && (qx & low) == 0) {  // the square's first pixel: inside whenever any of it is
            const uint32_t at = static_cast<uint32_t>(qy >> s) * static_cast<uint32_t>((W + low) >> s) + static_cast<uint32_t>(qx >> s);
            cell[at] = dm;
            cell[n_cells + at] = dp;
        }
        cell += 2 * n_cells;
    }
}

__global__ __launch_bounds__(kEncThreads) void encode_delta_kernel(const EncodeParams* slots, const DeltaParams* delta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const EncodeParams& Q = slots[blockIdx.y];
    const EntropyParams& P = Q.ep;
    const DeltaParams& D = delta[blockIdx.y];
    if (blockIdx.x >= Q.n_blocks) return;
    const int lane = threadIdx.x;
    const int n_grids = P.n_grids;
    int g = 0;
    while (g + 1 < n_grids && blockIdx.x >= Q.block_first[g + 1]) ++g;
    const int H = P.grid_h[g], W = P.grid_w[g], n = H * W;
    const int p = static_cast<int>(blockIdx.x - Q.block_first[g]) * kEncThreads + lane;
    if (p >= n) return;  // no cross-lane operation below
    const int8_t* __restrict__ lat = P.latent[g];
    float* __restrict__ out = D.map[g];
    const float inf = __builtin_inff();
    const int v = lat[p];
    if (!in_alphabet(v)) { out[p] = inf; out[n + p] = inf; return; }  // (the meter's launch set the slot's status)
    const int y = p / W, x = p - y * W;
    const bool has_m = v > kAcLo, has_p = v < kAcLo + kAlphabet - 1;

    // ---- its own symbol: the neighbouring symbols' intervals under the same (mu, rcp) ----
    double mu, rcp;
    encode_pixel_model<false>(P, g, y, x, lane, smem_raw, LatentOverride{}, mu, rcp);
    double am, ap;  // the sums for v - 1 and v + 1
    {
        const uint32_t l0 = window_left(mu, rcp, v - 1, kExpTab), l1 = window_left(mu, rcp, v, kExpTab);
        const uint32_t l2 = window_left(mu, rcp, v + 1, kExpTab), l3 = window_left(mu, rcp, v + 2, kExpTab);
        const double own = log2(static_cast<double>(l2 - l1));
        am = has_m ? own - log2(static_cast<double>(l1 - l0)) : 0.0;
        ap = has_p ? own - log2(static_cast<double>(l3 - l2)) : 0.0;
    }
    // ---- the pixels that have it as spatial tap k: (y + dy[k], x - dx[k]), the gather's signs turned round ----
    const int n_sp = P.n_spatial;
#pragma unroll 1
    for (int k = 0; k < n_sp; ++k) {
        const int qy = y + P.ctx_dy[k], qx = x - P.ctx_dx[k];
        if (qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
        const int sq = lat[qy * W + qx];
        if (!in_alphabet(sq)) continue;
        LatentOverride ov{g, y, x, v};
        double base = 0.0;
#pragma unroll 1
        for (int t = 0; t < 3; ++t) {  // as it is, v - 1, v + 1
            if ((t == 1 && !has_m) || (t == 2 && !has_p)) continue;
            ov.val = v + (t == 0 ? 0 : 2 * t - 3);
            encode_pixel_model<true>(P, g, qy, qx, lane, smem_raw, ov, mu, rcp);
            const double l = log2_width(mu, rcp, sq);
            if (t == 0) base = l;
            else if (t == 1) am += base - l;
            else ap += base - l;
        }
    }
    // ---- the finer grids whose IFCE feature reads it: grid gf has it as source channel g - gf - 1 ----
    for (int gf = 0; gf < g; ++gf) {
        const int c = g - gf - 1;
        if (P.ifce_in[gf] <= c) continue;
        const int hf = P.grid_h[gf], wf = P.grid_w[gf], base_level = P.level[gf + 1];
        const double* cell = D.partial + D.part_first[gf];
        for (int cc = 0; cc < c; ++cc) cell += 2 * delta_cells(hf, wf, delta_cell_shift(P.level[gf + 1 + cc] - base_level));
        const int sh = P.level[g] - base_level, s = delta_cell_shift(sh), r = sh + 1 - s;  // its block: 2^r x 2^r cells
        const int64_t nby = (hf + (1 << s) - 1) >> s, nbx = (wf + (1 << s) - 1) >> s;
        const int64_t by1 = min((static_cast<int64_t>(y) + 1) << r, nby), bx0 = static_cast<int64_t>(x) << r;
        const int64_t bx1 = min((static_cast<int64_t>(x) + 1) << r, nbx);
        for (int64_t by = static_cast<int64_t>(y) << r; by < by1; ++by)
            for (int64_t bx = bx0; bx < bx1; ++bx) {
                am += cell[by * nbx + bx];
                ap += cell[(nby + by) * nbx + bx];
            }
    }
    out[p] = has_m ? static_cast<float>(am) : inf;
    out[n + p] = has_p ? static_cast<float>(ap) : inf;
}

// ---- rate-network parameter deltas: what the slot's model bits would change by if ONE transmitted integer of the ARM (DESIGN.md
// 4.20) or of the IFCE (4.21) were v - 1 or v + 1.  Two launches behind the meter's, no atomics.
//   1. encode_rate_delta_kernel: blockIdx = (chunk, tile of 64 candidates, slot).  The wave walks the chunk's 64-pixel
//      workgroups in order; per workgroup one evaluation as it is, then one per candidate with the candidate's entry moved, the
//      width compared, and the lanes' log2(width) - log2(width'), width' - width and "moved" summed by wave_sum's fixed tree.
//      Lane c mod 64 keeps candidate c's running sums over the chunk's workgroups and stores the cell.  A workgroup in which no
//      lane's width moved adds nothing (its wave sums would be +0.0, 0, 0).
//   2. encode_rate_delta_final_kernel: one wave per candidate adds its cells lane-strided in chunk order and through the tree.
// The order of the additions of a candidate follows from the slot's geometry alone: not from the range of parameters asked for
// (which only decides the tile a candidate shares), the batch or the device.  Tail lanes and lanes whose symbol is outside the
// alphabet hold 0 and stay for the shuffles (the meter's launch set such a slot's status).
// What differs between the two networks (kKind), and nothing else:
//   a. the blocks walked: an IFCE candidate of grid g can only move symbols of grid g, and a block's grid is uniform, so the wave
//      walks only the blocks of the grids its tile's candidates name (they are sorted by grid: the first and the last give the range);
//   b. an IFCE candidate adds nothing for a block of another grid - which is what it would add there, no width moved;
//   c. what prices a lane: the generic path is a full encode_pixel_model<.., kKind> with the entry moved, the incremental path
//      arm_candidate or ifce_candidate on the kept state;
//   d. the row of the table a candidate answers: its own, or RateDeltaParams::row's for the sorted IFCE candidates.
// ---- the incremental path: the base evaluation's state stays in the LDS, a candidate is a rank-1 update of it ----
// Per-lane columns, [k][lane] like xa / xb: the inputs [dim], then every hidden layer's accumulators BEFORE the ReLU
// [n_hidden][dim], then - only for three hidden layers or more - two scratch columns [dim] each (armdelta_incremental_lds).
// The stabiliser's two sums and the output layer's two accumulators of the base are kept in registers (ArmBase).
struct ArmBase { uint64_t st0, st1, a0, a1; };
__device__ __forceinline__ int64_t relu16(int64_t v) { return (v < 0 ? 0 : v) >> 16; }
// input k of layer l (l == n_hidden: of the output layer) as the base evaluation has it
__device__ __forceinline__ int64_t arm_input(const int64_t* x0, int dim, int l, int k) {
    return l == 0 ? x0[k * kEncThreads] : relu16(x0[(l * dim + k) * kEncThreads]);  // layer l - 1's accumulators sit at column l * dim
}
// The base evaluation from the inputs in the first dim columns: armint.py:180-203, every accumulator stored.
__device__ __forceinline__ ArmBase arm_base_store(const EntropyParams& P, int64_t* x0) {
    const int dim = P.dim, n_hidden = P.n_layers - 1;
    const int64_t* ws = P.arm + (P.arm_len - 2 - 2 * dim);
    const int64_t* bs = ws + 2 * dim;
    ArmBase B{static_cast<uint64_t>(bs[0]), static_cast<uint64_t>(bs[1]), 0, 0};
    for (int k = 0; k < dim; ++k) {
        const uint64_t v = static_cast<uint64_t>(x0[k * kEncThreads]);
        B.st0 += v * static_cast<uint64_t>(ws[k * 2]);
        B.st1 += v * static_cast<uint64_t>(ws[k * 2 + 1]);
    }
    const int64_t* lw = P.arm;
    for (int l = 0; l < n_hidden; ++l) {
        const int64_t* lb = lw + dim * dim;
        int64_t* acc = x0 + (l + 1) * dim * kEncThreads;
        for (int o = 0; o < dim; o += 2) {
            const int o1 = min(o + 1, dim - 1);
            uint64_t a0 = static_cast<uint64_t>(lb[o]), a1 = static_cast<uint64_t>(lb[o1]);
            for (int k = 0; k < dim; ++k) {
                const uint64_t v = static_cast<uint64_t>(arm_input(x0, dim, l, k));
                a0 += v * static_cast<uint64_t>(lw[k * dim + o]);
                a1 += v * static_cast<uint64_t>(lw[k * dim + o1]);
            }
            acc[o * kEncThreads] = static_cast<int64_t>(a0);
            acc[o1 * kEncThreads] = static_cast<int64_t>(a1);
        }
        lw = lb + dim;
    }
    const int64_t* lb = lw + dim * 2;
    B.a0 = static_cast<uint64_t>(lb[0]); B.a1 = static_cast<uint64_t>(lb[1]);
    for (int k = 0; k < dim; ++k) {
        const uint64_t v = static_cast<uint64_t>(arm_input(x0, dim, n_hidden, k));
        B.a0 += v * static_cast<uint64_t>(lw[k * 2]);
        B.a1 += v * static_cast<uint64_t>(lw[k * 2 + 1]);
    }
    return B;
}
// Input `in` of layer l1 (l1 == n_hidden: of the output layer) moved by d: the layer's accumulators move by d * w[in][.] (re-rounded
// by their own ReLU), the layers behind it are recomputed in full through the two scratch columns sa and sa + dim columns; the last
// hidden layer's units go straight into the output layer's sums.  a0, a1: the output layer's two accumulators, the base's on
// entry.  sa is touched only when a hidden layer lies behind l1, the second column only when two do.
__device__ __forceinline__ void arm_input_moved(const EntropyParams& P, int64_t* x0, int l1, int in, uint64_t d, uint64_t& a0, uint64_t& a1, int64_t* sa) {
    const int dim = P.dim, n_hidden = P.n_layers - 1;
    const int64_t hidden_len = static_cast<int64_t>(dim) * dim + dim;
    const int64_t* wo = P.arm + n_hidden * hidden_len;  // the output layer: w[dim][2], b[2]
    if (l1 == n_hidden) {
        a0 += d * static_cast<uint64_t>(wo[in * 2]);
        a1 += d * static_cast<uint64_t>(wo[in * 2 + 1]);
        return;
    }
    const int64_t* lw = P.arm + l1 * hidden_len;
    const int64_t* acc = x0 + (l1 + 1) * dim * kEncThreads;
    int64_t* sb = sa + dim * kEncThreads;
    const bool last = l1 + 1 == n_hidden;
    if (last) { a0 = static_cast<uint64_t>(wo[2 * dim]); a1 = static_cast<uint64_t>(wo[2 * dim + 1]); }
    for (int o = 0; o < dim; ++o) {
        const int64_t v = relu16(static_cast<int64_t>(static_cast<uint64_t>(acc[o * kEncThreads]) + d * static_cast<uint64_t>(lw[in * dim + o])));
        if (last) {
            a0 += static_cast<uint64_t>(v) * static_cast<uint64_t>(wo[o * 2]);
            a1 += static_cast<uint64_t>(v) * static_cast<uint64_t>(wo[o * 2 + 1]);
        } else sa[o * kEncThreads] = v;
    }
    if (last) return;
    a0 = static_cast<uint64_t>(wo[2 * dim]); a1 = static_cast<uint64_t>(wo[2 * dim + 1]);
    for (int m = l1 + 1; m < n_hidden; ++m) {  // in full, as encode_pixel_model does
        const int64_t* mw = P.arm + m * hidden_len;
        const int64_t* mb = mw + dim * dim;
        const bool fold = m + 1 == n_hidden;  // (the sums are a ring: the order the units are added in does not matter)
        for (int o = 0; o < dim; ++o) {
            uint64_t t = static_cast<uint64_t>(mb[o]);
            for (int k = 0; k < dim; ++k) t += static_cast<uint64_t>(sa[k * kEncThreads]) * static_cast<uint64_t>(mw[k * dim + o]);
            const int64_t v = relu16(static_cast<int64_t>(t));
            if (fold) {
                a0 += static_cast<uint64_t>(v) * static_cast<uint64_t>(wo[o * 2]);
                a1 += static_cast<uint64_t>(v) * static_cast<uint64_t>(wo[o * 2 + 1]);
            } else sb[o * kEncThreads] = v;
        }
        int64_t* t = sa; sa = sb; sb = t;
    }
}
// The ARM's two sums with the candidate's entry moved.  Every step is the full evaluation's arithmetic modulo 2^64: the moved
// unit's accumulator changes by inc * input, its activation by delta, the next layer's accumulators by delta * weight (re-rounded
// by their own ReLU), the layers behind that are recomputed in full.  delta == 0: the base's sums.
__device__ __forceinline__ void arm_candidate(const EntropyParams& P, int64_t* x0, const ArmBase& B, const RateDeltaMove& pm, uint64_t& st0, uint64_t& st1) {
    const int dim = P.dim, n_hidden = P.n_layers - 1;
    uint64_t a0 = B.a0, a1 = B.a1;
    st0 = B.st0; st1 = B.st1;
    if (pm.at >= n_hidden) {  // output layer or stabiliser: one accumulator moves
        const bool stab = pm.at > n_hidden;
        const uint64_t c = static_cast<uint64_t>(pm.inc) * (pm.in < 0 ? uint64_t{1} : static_cast<uint64_t>(arm_input(x0, dim, stab ? 0 : n_hidden, pm.in)));
        if (pm.out == 0) a0 += c; else a1 += c;
    } else {
        const int l = pm.at;
        const uint64_t c = static_cast<uint64_t>(pm.inc) * (pm.in < 0 ? uint64_t{1} : static_cast<uint64_t>(arm_input(x0, dim, l, pm.in)));
        const int64_t a = x0[((l + 1) * dim + pm.out) * kEncThreads];
        const int64_t delta = relu16(static_cast<int64_t>(static_cast<uint64_t>(a) + c)) - relu16(a);
        if (delta != 0) arm_input_moved(P, x0, l + 1, pm.out, static_cast<uint64_t>(delta), a0, a1, x0 + (n_hidden + 1) * dim * kEncThreads);
    }
    st0 += a0; st1 += a1;
}

// The IFCE table's candidate on the same kept state: feature im.out of the pixel's grid is evaluated again with
// the candidate's entry moved (ifce_feature, fin multiply-adds).  Its change d in the << 16 input form moves the stabiliser's
// two sums by d * ws[n_sp + out][.] and ALL of layer 0's accumulators by d * w0[n_sp + out][.] - both exact in the ring - and
// every layer behind layer 0 is recomputed in full.  Of the kept state a candidate reads the inputs and layer 0's accumulators
// only, so the columns of the later layers' accumulators serve as the scratch.  d == 0: the base's sums.
__device__ __forceinline__ void ifce_candidate(const EntropyParams& P, int g, int y, int x, int64_t* x0, const ArmBase& B, const RateDeltaMove& im,
                                               uint64_t& st0, uint64_t& st1) {
    const int dim = P.dim, n_if = P.n_ifce_out, fin = P.ifce_in[g], row = P.n_spatial + im.out;
    const int64_t* fw_ = P.ifce + P.ifce_off[g];
    const bool first = g == P.n_grids - 1;
    const int64_t f = ifce_feature<false, true>(P, g, y >> 1, x >> 1, im.out, n_if, fin, first, first ? 0 : P.level[g + 1], fw_, fw_ + fin * n_if,
                                                LatentOverride{}, im);
    const uint64_t d = (static_cast<uint64_t>(f) << 16) - static_cast<uint64_t>(x0[row * kEncThreads]);
    uint64_t a0 = B.a0, a1 = B.a1;
    st0 = B.st0; st1 = B.st1;
    if (d != 0) {
        const int64_t* ws = P.arm + (P.arm_len - 2 - 2 * dim);
        st0 += d * static_cast<uint64_t>(ws[row * 2]);
        st1 += d * static_cast<uint64_t>(ws[row * 2 + 1]);
        // the scratch: the columns of layer 1's and layer 2's accumulators, which no IFCE candidate reads (ifcedelta_incremental_lds)
        arm_input_moved(P, x0, 0, row, d, a0, a1, x0 + 2 * dim * kEncThreads);
    }
    st0 += a0; st1 += a1;
}

// What one 64-pixel block adds to a candidate's running sums: the lanes' log2(width) - log2(width'), width' - width and "moved"
// through wave_sum's fixed tree, kept by the lane `mine` names.  A block in which no lane's width moved adds nothing (its wave sums
// would be +0.0, 0, 0).  Every lane of the wave calls it.
__device__ __forceinline__ void delta_block_sums(double d_bits, int64_t d_width, bool mine, ParamDeltaCell& acc) {
    const bool moved = d_width != 0;
    if (__ballot(moved) == 0) return;
    const double s_bits = wave_sum(d_bits);
    const uint64_t s_width = wave_sum(static_cast<uint64_t>(d_width)), s_moved = wave_sum(static_cast<uint64_t>(moved ? 1 : 0));
    if (mine) {
        acc.bits += s_bits;
        acc.sum_width += static_cast<int64_t>(s_width);
        acc.moved += static_cast<int64_t>(s_moved);
    }
}

// kKind: whose integers the table prices (kRateDeltaArm / kRateDeltaIfce; a. - c. above).  kIncremental: the slots whose path is the
// incremental one (RateDeltaParams::path); the other instantiation takes the rest.  Both give the same 64-bit words: the integer
// model is the same modulo 2^64, the floats and the order they are added in are this one function's.
template <int kKind, bool kIncremental>
__global__ __launch_bounds__(kEncThreads) void encode_rate_delta_kernel(const EncodeParams* slots, const RateDeltaParams* param) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const EncodeParams& Q = slots[blockIdx.z];
    const EntropyParams& P = Q.ep;
    const RateDeltaParams& D = param[blockIdx.z];
    const uint32_t chunk = blockIdx.x, c0 = blockIdx.y * kArmDeltaTile;
    if ((D.path == kArmDeltaIncremental) != kIncremental || chunk >= D.n_chunks || c0 >= D.n_cand) return;
    const int lane = threadIdx.x;
    const int n_grids = P.n_grids;
    const uint32_t nc = min(static_cast<uint32_t>(kArmDeltaTile), D.n_cand - c0);
    // a. the grids whose blocks the wave walks: all of them, or those the tile's candidates name (0 <= g <= g_hi < n_grids, ifcedelta_place)
    int g = 0, g_hi = n_grids - 1;
    if constexpr (kKind == kRateDeltaIfce) { g = D.cand[c0].at; g_hi = D.cand[c0 + nc - 1].at; }
    uint32_t b_first = chunk * kArmDeltaChunkBlocks;
    if constexpr (kKind == kRateDeltaIfce) b_first = max(b_first, Q.block_first[g]);
    const uint32_t b_end = min(min((chunk + 1) * static_cast<uint32_t>(kArmDeltaChunkBlocks), Q.n_blocks),
                               g_hi + 1 < n_grids ? Q.block_first[g_hi + 1] : Q.n_blocks);
    int64_t* x0 = reinterpret_cast<int64_t*>(smem_raw) + lane;
    ParamDeltaCell acc{0.0, 0, 0};  // of candidate c0 + lane
#pragma unroll 1
    for (uint32_t b = b_first; b < b_end; ++b) {
        while (g + 1 < n_grids && b >= Q.block_first[g + 1]) ++g;
        const int H = P.grid_h[g], W = P.grid_w[g];
        const int p = static_cast<int>(b - Q.block_first[g]) * kEncThreads + lane;
        const int sym = p < H * W ? P.latent[g][p] : 0;
        const bool ok = p < H * W && in_alphabet(sym);
        const int y = ok ? p / W : 0, x = ok ? p - y * W : 0;
        double mu, rcp, base = 0.0;
        uint32_t width = 0;
        ArmBase B{0, 0, 0, 0};
        if (ok) {
            if (kIncremental) {
                encode_pixel_model<false, kRateDeltaNone, true>(P, g, y, x, lane, smem_raw, LatentOverride{}, mu, rcp);
                B = arm_base_store(P, x0);
                arm_sums_to_model(P, B.st0 + B.a0, B.st1 + B.a1, mu, rcp);
            } else encode_pixel_model<false>(P, g, y, x, lane, smem_raw, LatentOverride{}, mu, rcp);
            width = window_left(mu, rcp, sym + 1, kExpTab) - window_left(mu, rcp, sym, kExpTab);
            base = log2(static_cast<double>(width));
        }
#pragma unroll 1
        for (uint32_t ci = 0; ci < nc; ++ci) {
            const RateDeltaMove mv = D.cand[c0 + ci];  // wave-uniform
            if (!mv.legal) continue;
            if constexpr (kKind == kRateDeltaIfce) if (mv.at != g) continue;  // b.
            double d_bits = 0.0;
            int64_t d_width = 0;
            if (ok) {
                if (kIncremental) {  // c.
                    uint64_t st0, st1;
                    if constexpr (kKind == kRateDeltaIfce) ifce_candidate(P, g, y, x, x0, B, mv, st0, st1);
                    else arm_candidate(P, x0, B, mv, st0, st1);
                    arm_sums_to_model(P, st0, st1, mu, rcp);
                } else encode_pixel_model<false, kKind>(P, g, y, x, lane, smem_raw, LatentOverride{}, mu, rcp, mv);
                const uint32_t w = window_left(mu, rcp, sym + 1, kExpTab) - window_left(mu, rcp, sym, kExpTab);
                if (w != width) {
                    d_bits = base - log2(static_cast<double>(w));
                    d_width = static_cast<int64_t>(w) - static_cast<int64_t>(width);
                }
            }
            delta_block_sums(d_bits, d_width, static_cast<uint32_t>(lane) == ci, acc);
        }
    }
    if (static_cast<uint32_t>(lane) < nc) D.partial[static_cast<size_t>(chunk) * D.n_cand + c0 + lane] = acc;
}

// blockIdx.x = candidate, blockIdx.y = slot; the cell is stored at the candidate's row (d. above).
__global__ __launch_bounds__(kEncThreads) void encode_rate_delta_final_kernel(const RateDeltaParams* param) {
    const RateDeltaParams& D = param[blockIdx.y];
    const uint32_t c = blockIdx.x;
    if (c >= D.n_cand) return;
    const int lane = threadIdx.x;
    double bits = 0.0;
    uint64_t width = 0, moved = 0;
    for (uint32_t j = lane; j < D.n_chunks; j += kEncThreads) {
        const ParamDeltaCell cell = D.partial[static_cast<size_t>(j) * D.n_cand + c];
        bits += cell.bits;
        width += static_cast<uint64_t>(cell.sum_width);
        moved += static_cast<uint64_t>(cell.moved);
    }
    bits = wave_sum(bits); width = wave_sum(width); moved = wave_sum(moved);
    if (lane != 0) return;
    const uint32_t r = D.row ? D.row[c] : c;  // wave-uniform
    if (D.cand[c].legal) D.out[r] = ParamDeltaCell{bits, static_cast<int64_t>(width), static_cast<int64_t>(moved)};
    else D.out[r] = ParamDeltaCell{static_cast<double>(__builtin_inff()), 0, 0};
}

size_t encode_contexts_lds_bytes(int dim) { return static_cast<size_t>(2) * dim * kEncThreads * sizeof(int64_t); }
int encode_block_threads() { return kEncThreads; }

hipError_t launch_encode(const EncodeParams* d_slots, int n_slots, unsigned max_blocks, size_t lds_bytes, hipStream_t stream) {
    if (n_slots <= 0) return hipSuccess;
    if (max_blocks > 0) {
        if (lds_bytes > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(encode_contexts_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes));
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(encode_contexts_kernel, dim3(max_blocks, n_slots), dim3(kEncThreads), lds_bytes, stream, d_slots);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(encode_chain_kernel, dim3(n_slots), dim3(kEncThreads), 0, stream, d_slots);
    return hipGetLastError();
}

hipError_t launch_encode_rate(const EncodeParams* d_slots, const RateParams* d_rate, int n_slots, unsigned max_blocks, int max_grids,
                              size_t lds_bytes, hipStream_t stream) {
    if (n_slots <= 0) return hipSuccess;
    if (max_blocks > 0) {
        if (lds_bytes > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(encode_rate_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes));
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(encode_rate_kernel, dim3(max_blocks, n_slots), dim3(kEncThreads), lds_bytes, stream, d_slots, d_rate);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (max_grids <= 0) return hipSuccess;
    hipLaunchKernelGGL(encode_rate_final_kernel, dim3(max_grids, n_slots), dim3(kEncThreads), 0, stream, d_slots, d_rate);
    return hipGetLastError();
}

hipError_t launch_encode_deltas(const EncodeParams* d_slots, const DeltaParams* d_delta, int n_slots, unsigned max_blocks,
                                unsigned max_tiles, size_t lds_bytes, hipStream_t stream) {
    if (n_slots <= 0 || max_blocks == 0) return hipSuccess;
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(encode_delta_ifce_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds_bytes));
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(encode_delta_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    static_cast<int>(lds_bytes));
        if (e != hipSuccess) return e;
    }
    if (max_tiles > 0) {
        hipLaunchKernelGGL(encode_delta_ifce_kernel, dim3(max_tiles, n_slots), dim3(kEncThreads), lds_bytes, stream, d_slots, d_delta);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(encode_delta_kernel, dim3(max_blocks, n_slots), dim3(kEncThreads), lds_bytes, stream, d_slots, d_delta);
    return hipGetLastError();
}

// One launch of the kind's table kernel per path that has slots (lds == 0: none; each workgroup of the other path's slots returns
// at once), then the final kernel.
hipError_t launch_encode_rate_deltas(int kind, const EncodeParams* d_slots, const RateDeltaParams* d_param, int n_slots, unsigned max_chunks,
                                     unsigned max_cand, size_t lds_generic, size_t lds_incremental, hipStream_t stream) {
    if (n_slots <= 0 || max_cand == 0) return hipSuccess;
    using Kernel = void (*)(const EncodeParams*, const RateDeltaParams*);
    static constexpr Kernel kernels[2][2] = {{encode_rate_delta_kernel<kRateDeltaArm, false>, encode_rate_delta_kernel<kRateDeltaArm, true>},
                                             {encode_rate_delta_kernel<kRateDeltaIfce, false>, encode_rate_delta_kernel<kRateDeltaIfce, true>}};
    const size_t lds[2] = {lds_generic, lds_incremental};
    const dim3 grid(max_chunks, (max_cand + kArmDeltaTile - 1) / kArmDeltaTile, n_slots);
    for (int path = 0; path < 2; ++path) {  // generic, incremental
        if (max_chunks == 0 || lds[path] == 0) continue;
        const Kernel kernel = kernels[kind == kRateDeltaIfce][path];
        if (lds[path] > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               static_cast<int>(lds[path]));
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kernel, grid, dim3(kEncThreads), lds[path], stream, d_slots, d_param);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(encode_rate_delta_final_kernel, dim3(max_cand, n_slots), dim3(kEncThreads), 0, stream, d_param);
    return hipGetLastError();
}

}  // namespace ccd
