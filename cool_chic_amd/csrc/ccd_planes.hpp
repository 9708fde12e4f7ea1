// ccd_planes.hpp - the sample step of the integer planes (decode.py:191-206 + png.py:57-58 / yuv.py:152-160), shared by the kernels
// that must agree bit for bit: planes_kernel (ccd_float.hip) and dsens_inter_kernel (ccd_inter.hip).
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
}  // namespace ccd
