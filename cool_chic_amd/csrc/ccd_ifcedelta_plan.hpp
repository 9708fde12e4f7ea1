// ccd_ifcedelta_plan.hpp - ccd_enc_measure_ifce_deltas: where IFCE integer k of a cool-chic (stream order, as decode_network
// takes them: the weights [n_ifce_out][fin_g] of every grid with input_features_ifce[g] > 0 in grid order, then the biases
// [n_ifce_out] of those grids) sits in the fixed-point IFCE block the kernels read (P.ifce + P.ifce_off[g]: w[fin][n_if], then
// b[n_if]), what "+1" is there, and which path prices it (host only, no HIP: tools/ifcedelta_host_check.cpp runs it under the
// sanitizers).  DESIGN.md 4.21.
#pragma once
#include <cstdint>

#include "../../include/ccd.h"
#include "ccd_armdelta_plan.hpp"

namespace ccd {

// One candidate as the kernel reads it.  For IFCE to_fixed_point is called with no -4, no residual unit and no inter-feature
// columns, and it is linear in every transmitted integer modulo 2^64: values[k] + s is one entry + s * 2^shift and nothing else.
struct IfceDeltaMove {
    int32_t grid;    // the grid whose feature moves: only symbols of this grid can change their interval
    int32_t out;     // feature 0 .. n_ifce_out - 1
    int32_t in;      // source channel 0 .. fin - 1 (grid `grid` + 1 + in); -1: the bias
    int32_t legal;   // 0: values[k] + s leaves int32 and cannot be transmitted
    int64_t inc;     // s * 2^shift, what the entry changes by
};
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

// Parameter k: its grid, feature and source channel, its place (*index into the grid's own block w[fin][n_if], b[n_if]) and the
// shift of "+1" (to_fixed_point's: 16 + q_w for a weight, 32 + q_b for a bias).  CCD_ERR_ARG for a k outside
// [0, ifcedelta_count), CCD_ERR_VALUE for a shift decode_network would refuse (< 0) or that is no 64-bit shift.
inline int ifcedelta_place(const IfceDeltaShape& s, int64_t k, IfceDeltaMove* mv, int64_t* index, int* shift) {
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
    mv->grid = g;
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

// The candidate (k, sign) of a network whose transmitted integer is `value`.
inline int ifcedelta_move(const IfceDeltaShape& s, int64_t k, int sign, int64_t value, IfceDeltaMove* mv, int64_t* index) {
    if (sign != -1 && sign != 1) return CCD_ERR_ARG;
    int shift = 0;
    const int rc = ifcedelta_place(s, k, mv, index, &shift);
    if (rc < 0) return rc;
    const int64_t moved = value + sign;
    mv->legal = moved >= INT32_MIN && moved <= INT32_MAX ? 1 : 0;
    const uint64_t unit = uint64_t{1} << shift;
    mv->inc = static_cast<int64_t>(sign < 0 ? uint64_t{0} - unit : unit);
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
// Which path prices a slot, by armdelta_path's rules and limit.
inline int ifcedelta_path(const IfceDeltaShape& s, int mode) {
    if (mode < kArmDeltaAuto || mode > kArmDeltaIncremental) return CCD_ERR_ARG;
    const bool fits = ifcedelta_incremental_lds(s) <= kArmDeltaMaxLds;
    if (mode == kArmDeltaIncremental) return fits ? kArmDeltaIncremental : CCD_ERR_UNSUPPORTED;
    return mode == kArmDeltaAuto && fits ? kArmDeltaIncremental : kArmDeltaGeneric;
}

}  // namespace ccd
