// ccd_ratedelta_plan.hpp - ccd_enc_measure_param_deltas and ccd_enc_measure_ifce_deltas: where transmitted integer k of a
// cool-chic's rate networks sits in the fixed-point network the kernels read, what "+1" is there, and which path prices it (host
// only, no HIP: tools/ratedelta_host_check.cpp runs it under the sanitizers).  DESIGN.md 4.20 (the ARM), 4.21 (the IFCE).
// Stream order, as decode_network takes the integers:
//   ARM:  the weights of every layer [out][in], the stabiliser's [2][dim], then the biases of every layer and the stabiliser's two;
//   IFCE: the weights [n_ifce_out][fin_g] of every grid with input_features_ifce[g] > 0 in grid order, then the biases
//         [n_ifce_out] of those grids.
// The two networks differ in the place of an integer (*_place), in their shapes and counts and in what the incremental path keeps
// per lane (*_incremental_lds); the candidate and the choice of the path are the same (ratedelta_move, ratedelta_path).
#pragma once
#include <cstdint>

#include "../../include/ccd.h"

namespace ccd {

// One candidate as the kernel reads it.  to_fixed_point is linear in every transmitted integer modulo 2^64, so values[k] + s is
// one entry + s * 2^shift and nothing else: the ARM's residual unit on the diagonal and the -4 of its last bias are constants
// beside it, and for the IFCE to_fixed_point is called with no -4, no residual unit and no inter-feature columns.
struct RateDeltaMove {
    int32_t at;      // ARM: the layer, 0 .. n_layers - 2 hidden, n_layers - 1 the output layer, n_layers the stabiliser;
                     // IFCE: the grid whose feature moves - only symbols of this grid can change their interval
    int32_t out;     // output unit of that layer; feature 0 .. n_ifce_out - 1
    int32_t in;      // input unit; source channel 0 .. fin - 1 (grid `at` + 1 + in); -1: the bias
    int32_t legal;   // 0: values[k] + s leaves int32 and cannot be transmitted
    int64_t inc;     // s * 2^shift, what the entry changes by
};
static_assert(sizeof(RateDeltaMove) == 24, "the candidate array's layout");

constexpr int kArmDeltaChunkBlocks = 32;  // 64-pixel blocks one wave of the table kernel walks
constexpr int kArmDeltaTile = 64;         // candidates one wave prices: lane c mod 64 keeps candidate c's sums
enum { kArmDeltaAuto = 0, kArmDeltaGeneric = 1, kArmDeltaIncremental = 2 };

// The candidate (k, sign) of an integer whose value is `value`: mv's place is the kind's *_place's, which also gave `shift`.
inline int ratedelta_move(int sign, int64_t value, int shift, RateDeltaMove* mv) {
    if (sign != -1 && sign != 1) return CCD_ERR_ARG;
    const int64_t moved = value + sign;
    mv->legal = moved >= INT32_MIN && moved <= INT32_MAX ? 1 : 0;
    const uint64_t unit = uint64_t{1} << shift;
    mv->inc = static_cast<int64_t>(sign < 0 ? uint64_t{0} - unit : unit);
    return CCD_OK;
}

// Which path prices a slot whose incremental state takes `lds` bytes for a wave (*_incremental_lds): kArmDeltaGeneric or
// kArmDeltaIncremental.  Where the state is beyond what a workgroup may take, the slot is priced by the generic path:
// CCD_ERR_UNSUPPORTED for mode 2 on such a slot, CCD_ERR_ARG for another mode.
constexpr int64_t kArmDeltaMaxLds = 160 * 1024;
inline int ratedelta_path(int64_t lds, int mode) {
    if (mode < kArmDeltaAuto || mode > kArmDeltaIncremental) return CCD_ERR_ARG;
    const bool fits = lds <= kArmDeltaMaxLds;
    if (mode == kArmDeltaIncremental) return fits ? kArmDeltaIncremental : CCD_ERR_UNSUPPORTED;
    return mode == kArmDeltaAuto && fits ? kArmDeltaIncremental : kArmDeltaGeneric;
}

// ---- the ARM: the fixed-point ARM is per layer w[in][out], b[out], then the stabiliser ws[dim][2], bs[2] (IntNetBlobs::arm) ----
struct ArmDeltaShape {
    int32_t dim, n_layers;  // inputs; hidden layers + 1
    int32_t n_ifce_out;     // the last n_ifce_out inputs are IFCE features (8 fractional bits less in layer 0 and the stabiliser)
    int32_t stabiliser;     // its integers are transmitted
    int32_t q_w, q_b;       // log2 of the weight and the bias step
};

inline ArmDeltaShape armdelta_shape(const ccd_cc_header& h) {
    return ArmDeltaShape{h.total_context_arm, h.n_hidden_layers_arm + 1, h.output_feature_ifce, h.linear_stabiliser_arm ? 1 : 0,
                         h.nn_q_step_log2[0], h.nn_q_step_log2[1]};
}
inline int64_t armdelta_n_weights(const ArmDeltaShape& s) {
    return static_cast<int64_t>(s.n_layers - 1) * s.dim * s.dim + 2 * static_cast<int64_t>(s.dim) + (s.stabiliser ? 2 * static_cast<int64_t>(s.dim) : 0);
}
inline int64_t armdelta_n_biases(const ArmDeltaShape& s) { return static_cast<int64_t>(s.n_layers - 1) * s.dim + 2 + (s.stabiliser ? 2 : 0); }
inline int64_t armdelta_count(const ArmDeltaShape& s) { return armdelta_n_weights(s) + armdelta_n_biases(s); }
// first entry of layer l (l == n_layers: the stabiliser) in the fixed-point ARM
inline int64_t armdelta_layer_first(const ArmDeltaShape& s, int l) {
    const int64_t hidden = static_cast<int64_t>(s.dim) * s.dim + s.dim;
    return l < s.n_layers ? l * hidden : (s.n_layers - 1) * hidden + 2 * static_cast<int64_t>(s.dim) + 2;
}

// Parameter k: its place (*index into the fixed-point ARM), the unit it belongs to and the shift of "+1" (to_fixed_point's:
// 16 + q_w, less 8 for the IFCE columns of layer 0 and of the stabiliser; 32 + q_b for a bias).  CCD_ERR_ARG for a k outside
// [0, armdelta_count), CCD_ERR_VALUE for a shift decode_network would refuse (< 0) or that is no 64-bit shift.
inline int armdelta_place(const ArmDeltaShape& s, int64_t k, RateDeltaMove* mv, int64_t* index, int* shift) {
    if (s.dim < 1 || s.n_layers < 1 || k < 0 || k >= armdelta_count(s)) return CCD_ERR_ARG;
    const int64_t n_w = armdelta_n_weights(s);
    int layer, out, in = -1;
    if (k < n_w) {
        const int64_t per = static_cast<int64_t>(s.dim) * s.dim;
        layer = static_cast<int>(k / per < s.n_layers - 1 ? k / per : s.n_layers - 1);
        int64_t r = k - layer * per;  // in the output layer's [2][dim], or past it in the stabiliser's
        if (layer == s.n_layers - 1 && r >= 2 * static_cast<int64_t>(s.dim)) { layer = s.n_layers; r -= 2 * static_cast<int64_t>(s.dim); }
        out = static_cast<int>(r / s.dim);
        in = static_cast<int>(r - static_cast<int64_t>(out) * s.dim);
    } else {
        const int64_t r = k - n_w;
        layer = static_cast<int>(r / s.dim < s.n_layers - 1 ? r / s.dim : s.n_layers - 1);
        int64_t o = r - static_cast<int64_t>(layer) * s.dim;
        if (layer == s.n_layers - 1 && o >= 2) { layer = s.n_layers; o -= 2; }
        out = static_cast<int>(o);
    }
    const int n_out = layer < s.n_layers - 1 ? s.dim : 2;
    int sh;
    if (in < 0) sh = 32 + s.q_b;
    else {
        sh = 16 + s.q_w;
        if (s.n_ifce_out > 0 && (layer == 0 || layer == s.n_layers) && in >= s.dim - s.n_ifce_out) sh -= 8;
    }
    if (sh < 0 || sh > 63) return CCD_ERR_VALUE;
    mv->at = layer; mv->out = out; mv->in = in;
    *index = armdelta_layer_first(s, layer) + (in < 0 ? static_cast<int64_t>(s.dim) * n_out + out : static_cast<int64_t>(in) * n_out + out);
    *shift = sh;
    return CCD_OK;
}

// Bytes of LDS the incremental path takes for a wave: per lane the inputs and every hidden layer's accumulators, and for three
// hidden layers or more two scratch columns for the layers recomputed in full.
inline int64_t armdelta_incremental_lds(const ArmDeltaShape& s) {
    const int n_hidden = s.n_layers - 1;
    return static_cast<int64_t>(1 + n_hidden + (n_hidden >= 3 ? 2 : 0)) * s.dim * 64 * 8;
}

// ---- the IFCE: the fixed-point block of grid g is w[fin][n_if], then b[n_if] (P.ifce + P.ifce_off[g]) ----
struct IfceDeltaShape {
    int32_t n_grids, n_ifce_out;
    int32_t fin[CCD_MAX_GRIDS];  // input_features_ifce: source channels of grid g, 0 = no IFCE there
    int32_t q_w, q_b;            // log2 of the IFCE weight and bias step
    ArmDeltaShape arm;           // the ARM behind the features: what the incremental path keeps per lane
};

inline IfceDeltaShape ifcedelta_shape(const ccd_cc_header& h) {
    IfceDeltaShape s{};
    s.n_grids = h.n_grids;
    s.n_ifce_out = h.output_feature_ifce;
    for (int g = 0; g < CCD_MAX_GRIDS; ++g) s.fin[g] = g < h.n_grids && h.output_feature_ifce > 0 ? h.input_features_ifce[g] : 0;
    s.q_w = h.nn_q_step_log2[2];
    s.q_b = h.nn_q_step_log2[3];
    s.arm = armdelta_shape(h);
    return s;
}
inline bool ifcedelta_shape_ok(const IfceDeltaShape& s) { return s.n_grids >= 0 && s.n_grids <= CCD_MAX_GRIDS && s.n_ifce_out >= 0; }
inline int64_t ifcedelta_n_weights(const IfceDeltaShape& s) {
    int64_t n = 0;
    for (int g = 0; g < s.n_grids; ++g) n += static_cast<int64_t>(s.n_ifce_out) * s.fin[g];
    return n;
}
inline int64_t ifcedelta_n_biases(const IfceDeltaShape& s) {
    int64_t n = 0;
    for (int g = 0; g < s.n_grids; ++g) n += s.fin[g] > 0 ? s.n_ifce_out : 0;
    return n;
}
inline int64_t ifcedelta_count(const IfceDeltaShape& s) { return ifcedelta_shape_ok(s) ? ifcedelta_n_weights(s) + ifcedelta_n_biases(s) : 0; }

// Parameter k: its grid, feature and source channel, its place (*index into the grid's own block) and the shift of "+1"
// (to_fixed_point's: 16 + q_w for a weight, 32 + q_b for a bias).  CCD_ERR_ARG for a k outside [0, ifcedelta_count),
// CCD_ERR_VALUE for a shift decode_network would refuse (< 0) or that is no 64-bit shift.
inline int ifcedelta_place(const IfceDeltaShape& s, int64_t k, RateDeltaMove* mv, int64_t* index, int* shift) {
    if (!ifcedelta_shape_ok(s) || k < 0 || k >= ifcedelta_count(s)) return CCD_ERR_ARG;
    const int64_t n_w = ifcedelta_n_weights(s);
    const int n_if = s.n_ifce_out;
    const bool bias = k >= n_w;
    int64_t r = bias ? k - n_w : k;
    int g = 0;
    for (;; ++g) {  // ends inside the grids: r < the sum of the blocks
        const int64_t block = s.fin[g] > 0 ? (bias ? n_if : static_cast<int64_t>(n_if) * s.fin[g]) : 0;
        if (r < block) break;
        r -= block;
    }
    const int sh = bias ? 32 + s.q_b : 16 + s.q_w;
    if (sh < 0 || sh > 63) return CCD_ERR_VALUE;
    mv->at = g;
    if (bias) {
        mv->out = static_cast<int>(r);
        mv->in = -1;
        *index = static_cast<int64_t>(s.fin[g]) * n_if + r;
    } else {  // the stream has [out][in], the block [in][out]
        mv->out = static_cast<int>(r / s.fin[g]);
        mv->in = static_cast<int>(r - static_cast<int64_t>(mv->out) * s.fin[g]);
        *index = static_cast<int64_t>(mv->in) * n_if + mv->out;
    }
    *shift = sh;
    return CCD_OK;
}

// Bytes of LDS the incremental path takes for a wave: per lane the ARM's inputs and every hidden layer's accumulators, as the
// ARM table's base evaluation leaves them.  A moved feature moves all of layer 0, so every layer behind layer 0 is recomputed in
// full, one layer earlier than behind a moved ARM entry: the scratch columns are needed from TWO hidden layers on (one; two from
// three on).  They cost nothing: a candidate reads the inputs and layer 0's accumulators only, so the columns of layer 1's and
// layer 2's accumulators - which exist exactly when the scratch is needed - are the scratch.
inline int64_t ifcedelta_incremental_lds(const IfceDeltaShape& s) {
    const int n_hidden = s.arm.n_layers - 1;
    return static_cast<int64_t>(1 + n_hidden) * s.arm.dim * 64 * 8;
}

}  // namespace ccd
