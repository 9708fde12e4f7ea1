// ccd_rdoq.hip - one RDOQ step: choose and apply +-1 moves of latents that provably do not interact (gfx950, wave64;
// DESIGN.md 4.14, include/ccd.h ccd_rdoq_*).
//
// A step is R rounds (ccd_rdoq_step_rounds; R = 1: ccd_rdoq_step).  A candidate is open, selected or blocked; a round lets the open
// ones compete, selects the winners and takes the cells of their boxes, and a candidate whose box holds a taken cell is blocked
// for good.  With fixed keys the rounds end at the set a walk over the candidates in key order would take.
//
// Inputs are the two delta maps of every grid (distortion: int64, rate: float32) and, per latent, its influence box in cells
// of the slot's claim raster (built on the host by the code behind ccd_rdoq_influence_box).  Two latents whose boxes share no
// cell neither share a symbol of the rate model nor a sample of the planes, so their deltas add.
//   rdoq_step_kernel<kSelect, kFirst, kFollow>   claim and select, one body (step_latent):
//     claim   round 0 (kFirst): the cost of both moves of a latent, its better move, whether that is a candidate, its 64-bit key
//             (cost as an ordered float, then the latent's number); later rounds: the open candidates, the same key.  An open
//             candidate with a taken cell in its box becomes blocked and claims nothing (round 0 has nothing to test: no cell is
//             taken yet); every other one does atomicMin of the key into every cell of its box.  The smallest key wins a cell
//             whatever the order of the atomics.
//     select  an open candidate that finds its own key in every cell of its box is selected: the latent is stored as v + s (a
//             byte store into the caller's grid), the move map gets s; round 0 gives every other latent's entry 0.
//   rdoq_settle_kernel<kFollow>   between two rounds, a lane per cell: a cell whose key belongs to a candidate selected in this
//             round becomes taken, and the claim word goes back to all ones.
//   rdoq_reduce_kernel<kFollow>   phase 0: a workgroup sums candidates, moves, open candidates, dD and dBits of one chunk of one
//             grid; phase 1: a wave per slot adds the chunks grid by grid, writes the result, stores all ones into the claim
//             raster and zeros into the taken raster.
// Work is dealt out by cells: a workgroup is one wave, and it is either 64 latents of one grid, a lane each, for boxes of
// up to kRdoqLaneCells cells, or ONE latent with a larger box (the grid's `big` list), the lanes over its cells.  Both are the
// same body, step_latent<kWave>: the box is walked by the three helpers set_taken / set_claim / set_mine, which deal its cells
// out with walk_cells<kWave>; the wave joins its lanes' answers with __any / __all and lets lane 0 store.  A workgroup finds its
// grid by bisection of a prefix table, as the dsens kernels do.
//
// The rasters.  claim needs all ones in the claim raster and the cells taken so far in the taken raster.  Inside one launch a
// word of either sees one kind of access: claim does plain loads of taken and atomics on the claim words; select does plain
// loads of the claim words; settle loads a claim word and the pick byte of its owner and stores the cell's two words, one lane
// per cell; phase 1 of the reduce launch, which follows the last round's select in place of a settle, stores every word of both
// rasters with plain vector stores.  Launches are ordered by their stream: no access of one launch meets one of another.  The
// first step finds what ccd_rdoq_add left: all ones and zeros.
//
// Groups.  The two slots of a linked pair (ccd_rdoq_link) share the leader's rasters: the follower's RdoqSlot carries the leader's
// raster / taken pointers and its grids the pair-wide uid (the leader's latents first), so claim and select are the code above
// with more candidates per word.  The smallest key still wins a cell whatever the order of the atomics: that never needed the
// claimants to be of one slot.  The accesses per word per launch stay of one kind too: claim and select reach a shared word
// from both slots, but with the same kind of access (atomics on claim words and loads of taken in claim, loads in select);
// settle runs over the cells of the rasters' owners only, one lane per cell, and finds the owner of a claimed word in the
// leader's grids or, from the follower's first uid on, in the follower's; in phase 1 of the reduce launch only the owner's
// wave stores the rasters (RdoqSlot::owns_raster), so no word is written by two workgroups.  The follower's own raster block
// stays as ccd_rdoq_add left it and is never read.
//
// Components (ccd_rdoq_follow).  A candidate of a following slot claims its CLAIM SET: its own box in its group's
// rasters and, per follow, its flow box in the rasters of the follow's target (RdoqSlotX / RdoqGridX, tables beside RdoqSlot /
// RdoqGrid that only the kFollow instantiations read).  The slots that links or follows connect share one numbering of their latents,
// so a key still names one candidate wherever it stands.  The rasters of a group are now reached from every slot of its
// component, and a word still sees one kind of access per launch: in claim, atomicMin on claim words and plain loads of taken,
// from any slot of the component; in select, plain loads of claim words; in settle, one lane per cell of the rasters' OWNER,
// which loads the claim word, looks its owner up by uid over the component's slots (a bisection of the component's first uids;
// the pick bytes it reads were last written by select, an earlier launch) and stores the cell's two words; in phase 1 of the
// reduce launch the owner's wave alone stores the rasters.  The reach tables see atomics in the reach launch and loads in the
// flow-box launch; a flow-box entry has one writer there and only readers afterwards.  Launches are ordered by their stream.
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

// A candidate no round has selected or blocked.
__device__ __forceinline__ bool is_open(uint32_t pick) { return pick != 0 && !(pick & (kRdoqSelected | kRdoqBlocked)); }

// Rule steps 1-3 for latent i of grid G.  Separate roundings of the two products and of the sum: what numpy float64 does.
// kFollow: the distortion is the own delta plus the dependent map's (X->dd_dep, where given), and a move exists in neither where
// either map holds the sentinel.
template <bool kFollow>
__device__ __forceinline__ Move best_move(const RdoqGrid& G, const RdoqSlot& S, const RdoqGridX* X, uint32_t i) {
    const int v = G.lat[i];
    double c64[2];
    bool exists[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        int64_t dd = G.dd ? G.dd[static_cast<size_t>(k) * G.n + i] : 0;
        const float db = G.db[static_cast<size_t>(k) * G.n + i];
        exists[k] = in_alphabet(v) && in_alphabet(v + 2 * k - 1) && dd != INT64_MIN && isfinite(db);
        if constexpr (kFollow) {
            if (X->dd_dep) {
                const int64_t dep = X->dd_dep[static_cast<size_t>(k) * G.n + i];
                exists[k] = exists[k] && dep != INT64_MIN;
                dd = static_cast<int64_t>(static_cast<uint64_t>(dd) + static_cast<uint64_t>(dep));
            }
        }
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

// A flow box in cells of the target's raster (congruent with the slot's own: ccd_rdoq_follow checked); empty: no cell.
__device__ __forceinline__ Cells flow_cells(const RdoqBox b, const RdoqSlot& S) {
    if (b.top > b.bottom || b.left > b.right) return Cells{0, 0, 0, 0, 0};
    return cells_of(b, S);
}
// The cells of a rectangle: all of them in this lane (kWave == false) or dealt out over the lanes of the wave.
template <bool kWave, typename Fn>
__device__ __forceinline__ void walk_cells(const Cells& c, uint32_t cells_w, uint32_t lane, Fn&& fn) {
    if (kWave) {
        for (uint32_t t = lane; t < c.n; t += 64) {
            const uint32_t r = t / c.bw, q = t - r * c.bw;
            fn(static_cast<size_t>(c.top + r) * cells_w + c.left + q);
        }
    } else {
        for (uint32_t r = 0; r < c.bh; ++r)
            for (uint32_t q = 0; q < c.bw; ++q) fn(static_cast<size_t>(c.top + r) * cells_w + c.left + q);
    }
}
// The rectangles of latent i's claim set with their rasters: its own box in its group's and, kFollow, its flow boxes in those of its
// follows' targets (X, SX: the entries beside G and S, null and never read otherwise).  fn answers for the own
// box whether the flow boxes are still to be walked: where the own box has decided, as for nearly every open candidate of a
// select, their tables are not even loaded.
template <bool kFollow, typename Fn>
__device__ __forceinline__ void claim_set(const Cells& own, const RdoqSlot& S, const RdoqGridX* X, const RdoqSlotX* SX, uint32_t i, Fn&& fn) {
    if (!fn(own, S.raster, S.taken)) return;
    if constexpr (kFollow)
        for (int k = 0; k < SX->n_follows; ++k) fn(flow_cells(X->fbox[k][i], S), SX->follow[k].raster, SX->follow[k].taken);
}
// Is a cell of the claim set taken, claim every cell, does the key stand in every cell.  In a wave the answer is this lane's share.
template <bool kWave, bool kFollow>
__device__ __forceinline__ bool set_taken(const Cells& own, const RdoqSlot& S, const RdoqGridX* X, const RdoqSlotX* SX, uint32_t i, uint32_t lane) {
    bool hit = false;
    claim_set<kFollow>(own, S, X, SX, i, [&](const Cells& c, const unsigned long long*, const uint8_t* taken) {
        walk_cells<kWave>(c, S.cells_w, lane, [&](size_t at) { hit = hit || taken[at] != 0; });
        return !hit;
    });
    return hit;
}
template <bool kWave, bool kFollow>
__device__ __forceinline__ void set_claim(const Cells& own, const RdoqSlot& S, const RdoqGridX* X, const RdoqSlotX* SX, uint32_t i, uint32_t lane,
                                          unsigned long long key) {
    claim_set<kFollow>(own, S, X, SX, i, [&](const Cells& c, unsigned long long* raster, const uint8_t*) {
        walk_cells<kWave>(c, S.cells_w, lane, [&](size_t at) { atomicMin(&raster[at], key); });
        return true;
    });
}
template <bool kWave, bool kFollow>
__device__ __forceinline__ bool set_mine(const Cells& own, const RdoqSlot& S, const RdoqGridX* X, const RdoqSlotX* SX, uint32_t i, uint32_t lane,
                                         unsigned long long key) {
    bool mine = true;
    claim_set<kFollow>(own, S, X, SX, i, [&](const Cells& c, const unsigned long long* raster, const uint8_t*) {
        walk_cells<kWave>(c, S.cells_w, lane, [&](size_t at) { mine = mine && raster[at] == key; });
        return mine;
    });
    return mine;
}

// One body for both work splits.  kWave == false: a lane per latent, 64 latents of one grid per workgroup; kWave == true: one
// latent of a `big` list, the lanes over the cells of its claim set - every lane reads the pick byte and the latent (best_move)
// before lane 0 stores either (one wave, program order), the lanes' answers meet in __any / __all, and lane 0 alone stores.
// kSelect == false: claim.  kSelect == true: select and apply.  Round 0 (kFirst) finds the candidates; a later round reads their
// state from the pick bytes and forms an open candidate's key again: its latent and the maps are what they were.
// kFollow: "the box" is the claim set (claim_set above).
template <bool kWave, bool kSelect, bool kFirst, bool kFollow>
__device__ __forceinline__ void step_latent(const RdoqGrid& G, const RdoqSlot& S, const RdoqGridX* __restrict__ X, const RdoqSlotX* __restrict__ SX,
                                            uint32_t i) {
    const uint32_t lane = threadIdx.x;
    if (i >= G.n) return;
    const Cells c = cells_of(G.box[i], S);
    if (!kWave && c.n > kRdoqLaneCells) return;  // a wave's
    const bool stores = !kWave || lane == 0;
    if constexpr (!kSelect) {
        uint32_t pick = kFirst ? 0 : G.pick[i];
        if (!kFirst && !is_open(pick)) return;  // (in a wave: the same in every lane)
        const Move m = best_move<kFollow>(G, S, X, i);
        if (kFirst) pick = static_cast<uint32_t>(m.pick);
        bool blocked = false;
        if constexpr (!kFirst) {  // (no cell is taken before the first round)
            blocked = set_taken<kWave, kFollow>(c, S, X, SX, i, lane);
            if constexpr (kWave) blocked = __any(blocked);
        }
        if (blocked) pick |= kRdoqBlocked;
        if (stores && (kFirst || blocked)) G.pick[i] = static_cast<uint8_t>(pick);
        if (pick && !blocked) set_claim<kWave, kFollow>(c, S, X, SX, i, lane, m.key);
    } else {
        int s = 0;
        const uint32_t pick = G.pick[i];
        if (is_open(pick)) {  // (in a wave: the same in every lane)
            const Move m = best_move<kFollow>(G, S, X, i);
            bool mine = set_mine<kWave, kFollow>(c, S, X, SX, i, lane, m.key);
            if constexpr (kWave) mine = __all(mine);
            if (mine) s = m.s;
            if (stores && s) {
                G.lat[i] = static_cast<int8_t>(G.lat[i] + s);
                G.pick[i] = static_cast<uint8_t>(pick | kRdoqSelected);
            }
        }
        if (stores && (kFirst || s)) G.moves[i] = static_cast<int8_t>(s);
    }
}

// Every table a kernel reads is a __restrict__ pointer argument of the kernel itself: through a by-value struct of the same pointers
// (measured: profiles/r14) the compiler can no longer prove that the kernel's stores leave the tables alone, and the bisection of
// the prefix table, a chain of dependent loads in front of everything a workgroup does, turns from scalar into vector loads.

// Which latent a workgroup's lanes work on: lane i of 64 latents of a grid, or all lanes on one entry of a `big` list.
template <bool kWave, bool kSelect, bool kFirst, bool kFollow>
__device__ __forceinline__ void step_body(const RdoqGrid* __restrict__ grids, const RdoqSlot* __restrict__ slots,
                                          const uint32_t* __restrict__ lane_prefix, const uint32_t* __restrict__ big_prefix, int n_grids,
                                          uint32_t n_lane_blocks, const RdoqGridX* __restrict__ gx, const RdoqSlotX* __restrict__ sx) {
    const uint32_t u = kWave ? blockIdx.x - n_lane_blocks : blockIdx.x;
    const int e = entry_of(kWave ? big_prefix : lane_prefix, n_grids, u);
    const RdoqGrid& G = grids[e];
    const uint32_t i = kWave ? G.big[u - big_prefix[e]] : (u - lane_prefix[e]) * 64u + threadIdx.x;
    step_latent<kWave, kSelect, kFirst, kFollow>(G, slots[G.slot], kFollow ? gx + e : nullptr, kFollow ? sx + G.slot : nullptr, i);
}

// kFirst: the kernels of round 0, all that a step of one round runs before the sums.  kFollow: the same body over
// claim sets; without it gx / sx are null and never read.
template <bool kSelect, bool kFirst, bool kFollow>
__global__ __launch_bounds__(64) void rdoq_step_kernel(const RdoqGrid* __restrict__ grids, const RdoqSlot* __restrict__ slots,
                                                       const uint32_t* __restrict__ lane_prefix, const uint32_t* __restrict__ big_prefix,
                                                       int n_grids, uint32_t n_lane_blocks, const RdoqGridX* __restrict__ gx,
                                                       const RdoqSlotX* __restrict__ sx) {
    if (blockIdx.x < n_lane_blocks) step_body<false, kSelect, kFirst, kFollow>(grids, slots, lane_prefix, big_prefix, n_grids, n_lane_blocks, gx, sx);
    else step_body<true, kSelect, kFirst, kFollow>(grids, slots, lane_prefix, big_prefix, n_grids, n_lane_blocks, gx, sx);
}

// The flow box of every latent of a following slot, per follow: the bounding rectangle of reach[c] over the cells c of the
// latent's own box, from the reach tables the launch before this one built.  The split of the step's kernels: a
// lane per latent with a box of up to kRdoqLaneCells cells, a wave per latent of the `big` lists.  Every entry has one writer.
__device__ __forceinline__ void reach_min(uint4& m, const uint32_t* __restrict__ reach, size_t at) {
    const uint4 w = reinterpret_cast<const uint4*>(reach)[at];
    m.x = min(m.x, w.x); m.y = min(m.y, w.y); m.z = min(m.z, w.z); m.w = min(m.w, w.w);
}
__device__ __forceinline__ RdoqBox flow_box_of(const uint4 m) {
    RdoqBox b = {0xffff, 0xffff, 0, 0};  // empty
    if (m.x != ~0u) {
        b.top = static_cast<uint16_t>(m.x); b.left = static_cast<uint16_t>(m.y);
        b.bottom = static_cast<uint16_t>(~m.z); b.right = static_cast<uint16_t>(~m.w);
    }
    return b;
}
__global__ __launch_bounds__(64) void rdoq_flowbox_kernel(const RdoqGrid* __restrict__ grids, const RdoqSlot* __restrict__ slots,
                                                          const uint32_t* __restrict__ lane_prefix, const uint32_t* __restrict__ big_prefix,
                                                          int n_grids, uint32_t n_lane_blocks, const RdoqGridX* __restrict__ gx,
                                                          const RdoqSlotX* __restrict__ sx) {
    const uint32_t lane = threadIdx.x;
    const bool wave = blockIdx.x >= n_lane_blocks;
    const uint32_t u = blockIdx.x - n_lane_blocks;
    const int e = wave ? entry_of(big_prefix, n_grids, u) : entry_of(lane_prefix, n_grids, blockIdx.x);
    const RdoqGrid& G = grids[e];
    const RdoqSlot& S = slots[G.slot];
    const RdoqSlotX& SX = sx[G.slot];
    const RdoqGridX& X = gx[e];
    if (SX.n_follows == 0) return;
    const uint32_t i = wave ? G.big[u - big_prefix[e]] : (blockIdx.x - lane_prefix[e]) * 64u + lane;
    if (i >= G.n) return;
    const Cells c = cells_of(G.box[i], S);
    if (!wave && c.n > kRdoqLaneCells) return;  // a wave's
    for (int k = 0; k < SX.n_follows; ++k) {
        uint4 m = make_uint4(~0u, ~0u, ~0u, ~0u);
        const uint32_t* reach = SX.follow[k].reach;
        if (wave) {
            walk_cells<true>(c, S.cells_w, lane, [&](size_t at) { reach_min(m, reach, at); });
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                m.x = min(m.x, __shfl_xor(m.x, off, 64)); m.y = min(m.y, __shfl_xor(m.y, off, 64));
                m.z = min(m.z, __shfl_xor(m.z, off, 64)); m.w = min(m.w, __shfl_xor(m.w, off, 64));
            }
            if (lane == 0) X.fbox[k][i] = flow_box_of(m);
        } else {
            walk_cells<false>(c, S.cells_w, lane, [&](size_t at) { reach_min(m, reach, at); });
            X.fbox[k][i] = flow_box_of(m);
        }
    }
}

// Between two rounds: 64 cells of one raster, a lane each (a follower has no cell blocks: its leader's lanes settle the pair's
// raster).  The low half of a claimed word is its owner's uid; the owner claimed in this round, so a selected owner was selected
// in this round and owns every cell of its box.  In a pair the owner is a latent of either slot: the follower's uids begin where
// the leader's end.
// kFollow: the owner is a latent of any slot of the raster owner's component; its slot is the last entry of the component's
// table of first uids that is not above the uid (a bisection; the partner test is its two-slot case).
template <bool kFollow>
__global__ __launch_bounds__(64) void rdoq_settle_kernel(const RdoqGrid* __restrict__ grids, const RdoqSlot* __restrict__ slots,
                                                         const uint32_t* __restrict__ cell_prefix, int n_slots, const RdoqSlotX* __restrict__ sx,
                                                         const uint32_t* __restrict__ comp_uid, const int32_t* __restrict__ comp_slot) {
    const int k = entry_of(cell_prefix, n_slots, blockIdx.x);
    const RdoqSlot& S = slots[k];
    const size_t cell = static_cast<size_t>(blockIdx.x - cell_prefix[k]) * 64u + threadIdx.x;
    if (cell >= static_cast<size_t>(S.cells_h) * S.cells_w) return;
    const unsigned long long key = S.raster[cell];
    if (key == ~0ull) return;  // nobody claimed the cell
    const uint32_t uid = static_cast<uint32_t>(key);
    const RdoqSlot* O = &S;  // the slot of the uid
    if constexpr (kFollow) {
        int lo = sx[k].comp_first, hi = lo + sx[k].comp_n - 1;  // comp_uid[lo] == 0 <= uid
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (comp_uid[mid] <= uid) lo = mid; else hi = mid - 1;
        }
        O = &slots[comp_slot[lo]];
    } else if (S.partner >= 0 && grids[slots[S.partner].first_grid].first <= uid) O = &slots[S.partner];
    int g = 0;  // the grid of the uid: first[] ascends over the slot's few grids
    while (g + 1 < O->n_grids && grids[O->first_grid + g + 1].first <= uid) ++g;
    const RdoqGrid& G = grids[O->first_grid + g];
    const uint32_t i = uid - G.first;
    if (i < G.n && (G.pick[i] & kRdoqSelected)) S.taken[cell] = 1;
    S.raster[cell] = ~0ull;
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

// kFollow: the chosen entries of the dependent maps are summed beside d_sse (integers, any order): partial_dep per chunk, then
// dep_out per slot.
template <bool kFollow>
__global__ __launch_bounds__(64) void rdoq_reduce_kernel(const RdoqGrid* __restrict__ grids, const RdoqSlot* __restrict__ slots,
                                                         const uint32_t* __restrict__ chunk_prefix, int n_grids, const RdoqSums O, int phase,
                                                         const RdoqGridX* __restrict__ gx) {
    const uint32_t lane = threadIdx.x;
    RdoqPartial acc = {0, 0, 0, 0.0, 0};
    int64_t dep = 0;
    if (phase == 0) {
        const int e = entry_of(chunk_prefix, n_grids, blockIdx.x);
        const RdoqGrid& G = grids[e];
        const uint32_t i0 = (blockIdx.x - chunk_prefix[e]) * kRdoqChunk;
        const uint32_t i1 = min(i0 + kRdoqChunk, G.n);
        for (uint32_t i = i0 + lane; i < i1; i += 64) {
            const uint32_t pick = G.pick[i];
            acc.n_candidates += pick != 0;
            acc.n_open += is_open(pick);  // it took part in the last round and lost a cell
            const int s = G.moves[i];
            if (s == 0) continue;
            const size_t at = (s > 0 ? static_cast<size_t>(G.n) : 0) + i;
            acc.n_moves += 1;
            acc.d_sse += G.dd ? G.dd[at] : 0;
            acc.d_bits = __dadd_rn(acc.d_bits, static_cast<double>(G.db[at]));
            if constexpr (kFollow)
                if (gx[e].dd_dep) dep += gx[e].dd_dep[at];
        }
    } else {
        const RdoqSlot& S = slots[blockIdx.x];
        ccd_rdoq_result& R = O.results[blockIdx.x];
        RdoqPartial total = {0, 0, 0, 0.0, 0};
        if constexpr (kFollow) {
            for (uint32_t c = chunk_prefix[S.first_grid] + lane; c < chunk_prefix[S.first_grid + S.n_grids]; c += 64) dep += O.partial_dep[c];
            dep = wave_sum_i64(dep);
            if (lane == 0) O.dep_out[blockIdx.x] = dep;
        }
        for (int g = 0; g < S.n_grids; ++g) {
            const int e = S.first_grid + g;
            acc = {0, 0, 0, 0.0, 0};
            for (uint32_t c = chunk_prefix[e] + lane; c < chunk_prefix[e + 1]; c += 64) {
                const RdoqPartial P = O.partial[c];
                acc.n_candidates += P.n_candidates;
                acc.n_moves += P.n_moves;
                acc.d_sse += P.d_sse;
                acc.d_bits = __dadd_rn(acc.d_bits, P.d_bits);
                acc.n_open += P.n_open;
            }
            acc.n_candidates = wave_sum_i64(acc.n_candidates);
            acc.n_moves = wave_sum_i64(acc.n_moves);
            acc.d_sse = wave_sum_i64(acc.d_sse);
            acc.d_bits = wave_sum_f64(acc.d_bits);
            acc.n_open = wave_sum_i64(acc.n_open);
            if (lane == 0) R.n_moves_grid[g] = acc.n_moves;
            total.n_candidates += acc.n_candidates;
            total.n_moves += acc.n_moves;
            total.d_sse += acc.d_sse;
            total.d_bits = __dadd_rn(total.d_bits, acc.d_bits);
            total.n_open += acc.n_open;
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
            O.open[blockIdx.x] = total.n_open;
        }
        // all ones and no taken cell for the next step's claim (the ordering argument is at the head of this file); a pair's
        // rasters are the leader's to store
        if (!S.owns_raster) return;
        uint4* words = reinterpret_cast<uint4*>(S.raster);
        for (uint32_t t = lane; t < S.raster_units; t += 64) words[t] = make_uint4(~0u, ~0u, ~0u, ~0u);
        uint4* marks = reinterpret_cast<uint4*>(S.taken);
        for (uint32_t t = lane; t < S.taken_units; t += 64) marks[t] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    acc.n_candidates = wave_sum_i64(acc.n_candidates);
    acc.n_moves = wave_sum_i64(acc.n_moves);
    acc.d_sse = wave_sum_i64(acc.d_sse);
    acc.d_bits = wave_sum_f64(acc.d_bits);
    acc.n_open = wave_sum_i64(acc.n_open);
    if (lane == 0) O.partial[blockIdx.x] = acc;
    if constexpr (kFollow) {
        dep = wave_sum_i64(dep);
        if (lane == 0) O.partial_dep[blockIdx.x] = dep;
    }
}
// `rounds` times claim, select (and settle between two rounds: after the last round phase 1 of the reduce launch writes both
// rasters), then the two phases of the reduce launch: 3 R + 1 launches.
template <bool kFollow>
hipError_t launch_rounds(const RdoqStepLaunch& L, hipStream_t stream) {
    const RdoqStepTables& T = L.t;
    const dim3 units(T.n_lane_blocks + L.n_big), wave(64);
    for (int k = 0; k < L.rounds; ++k) {
        hipLaunchKernelGGL((k == 0 ? rdoq_step_kernel<false, true, kFollow> : rdoq_step_kernel<false, false, kFollow>), units, wave, 0, stream, T.grids,
                           T.slots, T.lane_prefix, T.big_prefix, T.n_grids, T.n_lane_blocks, T.gx, T.sx);
        hipLaunchKernelGGL((k == 0 ? rdoq_step_kernel<true, true, kFollow> : rdoq_step_kernel<true, false, kFollow>), units, wave, 0, stream, T.grids,
                           T.slots, T.lane_prefix, T.big_prefix, T.n_grids, T.n_lane_blocks, T.gx, T.sx);
        if (k + 1 < L.rounds)
            hipLaunchKernelGGL(rdoq_settle_kernel<kFollow>, dim3(L.n_cell_blocks), wave, 0, stream, T.grids, T.slots, T.cell_prefix, T.n_slots, T.sx,
                               T.comp_uid, T.comp_slot);
    }
    hipLaunchKernelGGL(rdoq_reduce_kernel<kFollow>, dim3(L.n_chunks), wave, 0, stream, T.grids, T.slots, T.chunk_prefix, T.n_grids, L.sums, 0, T.gx);
    hipLaunchKernelGGL(rdoq_reduce_kernel<kFollow>, dim3(T.n_slots), wave, 0, stream, T.grids, T.slots, T.chunk_prefix, T.n_grids, L.sums, 1, T.gx);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_rdoq_step(const RdoqStepLaunch& L, hipStream_t stream) {
    if (L.t.n_grids <= 0 || L.t.n_slots <= 0 || L.t.n_lane_blocks == 0 || L.n_chunks == 0 || L.n_cell_blocks == 0 || L.rounds < 1) return hipSuccess;
    if (!L.t.gx) return launch_rounds<false>(L, stream);
    // the variants over claim sets: one memset, the reach launch(es) and the flow boxes in front of the rounds
    if (L.n_reach[0] + L.n_reach[1] > 0) {
        if (L.stages & 1) {
            hipError_t e = hipMemsetAsync(L.reach_mem, 0xff, L.reach_bytes, stream);
            for (int c = 0; c < 2 && e == hipSuccess; ++c) e = launch_rdoq_reach(L.reach_jobs[c], L.reach_prefix[c], L.n_reach[c], L.reach_blocks[c], c, stream);
            if (e != hipSuccess) return e;
        }
        if (L.stages & 2)
            hipLaunchKernelGGL(rdoq_flowbox_kernel, dim3(L.t.n_lane_blocks + L.n_big), dim3(64), 0, stream, L.t.grids, L.t.slots, L.t.lane_prefix,
                               L.t.big_prefix, L.t.n_grids, L.t.n_lane_blocks, L.t.gx, L.t.sx);
    }
    if (!(L.stages & 4)) return hipGetLastError();  // (a timing run of the tables alone: no result is written)
    return launch_rounds<true>(L, stream);
}
}  // namespace ccd
