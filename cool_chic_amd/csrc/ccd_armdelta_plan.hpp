// ccd_armdelta_plan.hpp - ccd_enc_measure_param_deltas: where parameter k of a cool-chic's ARM (stream order: the weights of
// every layer [out][in], the stabiliser's [2][dim], then the biases of every layer and the stabiliser's two) sits in the
// fixed-point ARM the kernels read, what "+1" is there, and which path prices it (host only, no HIP:
// tools/armdelta_host_check.cpp runs it under the sanitizers).  DESIGN.md 4.20.
#pragma once
#include <cstdint>

#include "../../include/ccd.h"

namespace ccd {

// One candidate as the kernel reads it.  The fixed-point ARM is per layer w[in][out], b[out], then the stabiliser ws[dim][2],
// bs[2] (IntNetBlobs::arm); to_fixed_point is linear in every transmitted integer modulo 2^64, so values[k] + s is entry
// `index` + s * 2^shift and nothing else: the residual unit on the diagonal and the -4 of the last bias are constants beside it.
struct ArmDeltaMove {
    int32_t layer;   // 0 .. n_layers - 2 hidden, n_layers - 1 the output layer, n_layers the stabiliser
    int32_t out;     // output unit of that layer
    int32_t in;      // input unit; -1: the bias
    int32_t legal;   // 0: values[k] + s leaves int32 and cannot be transmitted
    int64_t inc;     // s * 2^shift, what the entry changes by
};
struct ArmDeltaShape {
    int32_t dim, n_layers;  // inputs; hidden layers + 1
    int32_t n_ifce_out;     // the last n_ifce_out inputs are IFCE features (8 fractional bits less in layer 0 and the stabiliser)
    int32_t stabiliser;     // its integers are transmitted
    int32_t q_w, q_b;       // log2 of the weight and the bias step
};

constexpr int kArmDeltaChunkBlocks = 32;  // 64-pixel blocks one wave of the table kernel walks
constexpr int kArmDeltaTile = 64;         // candidates one wave prices: lane c mod 64 keeps candidate c's sums
enum { kArmDeltaAuto = 0, kArmDeltaGeneric = 1, kArmDeltaIncremental = 2 };

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
inline int armdelta_place(const ArmDeltaShape& s, int64_t k, ArmDeltaMove* mv, int64_t* index, int* shift) {
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
    mv->layer = layer; mv->out = out; mv->in = in;
    *index = armdelta_layer_first(s, layer) + (in < 0 ? static_cast<int64_t>(s.dim) * n_out + out : static_cast<int64_t>(in) * n_out + out);
    *shift = sh;
    return CCD_OK;
}

// The candidate (k, sign) of a network whose transmitted integer is `value`.
inline int armdelta_move(const ArmDeltaShape& s, int64_t k, int sign, int64_t value, ArmDeltaMove* mv, int64_t* index) {
    if (sign != -1 && sign != 1) return CCD_ERR_ARG;
    int shift = 0;
    const int rc = armdelta_place(s, k, mv, index, &shift);
    if (rc < 0) return rc;
    const int64_t moved = value + sign;
    mv->legal = moved >= INT32_MIN && moved <= INT32_MAX ? 1 : 0;
    const uint64_t unit = uint64_t{1} << shift;
    mv->inc = static_cast<int64_t>(sign < 0 ? uint64_t{0} - unit : unit);
    return CCD_OK;
}

// Bytes of LDS the incremental path takes for a wave: per lane the inputs and every hidden layer's accumulators, and for three
// hidden layers or more two scratch columns for the layers recomputed in full.  Where that is beyond what a workgroup may
// take, the slot is priced by the generic path.
constexpr int64_t kArmDeltaMaxLds = 160 * 1024;
inline int64_t armdelta_incremental_lds(const ArmDeltaShape& s) {
    const int n_hidden = s.n_layers - 1;
    return static_cast<int64_t>(1 + n_hidden + (n_hidden >= 3 ? 2 : 0)) * s.dim * 64 * 8;
}
// Which path prices a slot: kArmDeltaGeneric or kArmDeltaIncremental; CCD_ERR_UNSUPPORTED for mode 2 on a slot whose state
// does not fit, CCD_ERR_ARG for another mode.
inline int armdelta_path(const ArmDeltaShape& s, int mode) {
    if (mode < kArmDeltaAuto || mode > kArmDeltaIncremental) return CCD_ERR_ARG;
    const bool fits = armdelta_incremental_lds(s) <= kArmDeltaMaxLds;
    if (mode == kArmDeltaIncremental) return fits ? kArmDeltaIncremental : CCD_ERR_UNSUPPORTED;
    return mode == kArmDeltaAuto && fits ? kArmDeltaIncremental : kArmDeltaGeneric;
}

}  // namespace ccd
