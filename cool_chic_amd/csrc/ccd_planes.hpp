// ccd_planes.hpp - the sample step of the integer planes (decode.py:191-206 + png.py:57-58 / yuv.py:152-160), shared by the kernels
// that must agree bit for bit: planes_kernel (ccd_float.hip), syn_fused_kernel (ccd_synth_fused.hip), dsens_inter_kernel,
// dsens_dep_kernel and inter_score_kernel (ccd_inter.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ccd {
__device__ __forceinline__ float round_to_grid(float x, float maxv) { return rintf(maxv * x) / maxv; }

__device__ __forceinline__ unsigned quantise_sample(float x, float maxv) {
    float q = round_to_grid(x, maxv);
    q = q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q);
    q = rintf(q * maxv) / maxv;
    return static_cast<unsigned>(rintf(q * maxv));
}

// a 4:2:0 chroma sample from `sum`, the sequential f32 sum of the 2 x 2 window's round_to_grid samples (dy outer, dx inner):
// F.avg_pool2d(kernel 2, stride 2), yuv.py:295, then clamp, round to the grid, round
__device__ __forceinline__ unsigned quantise_chroma420(float sum, float maxv) {
    float a = sum / 4.0f;
    a = a < 0.0f ? 0.0f : (a > 1.0f ? 1.0f : a);
    a = rintf(a * maxv) / maxv;
    return static_cast<unsigned>(rintf(a * maxv));
}
}  // namespace ccd
