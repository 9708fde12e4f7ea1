// ccd_trig.hpp - sin / cos in f64 as oracle/cc_oracle.c evaluates them (sections 9c and 11: fixed fma chains over a two-constant
// reduction by pi / 2), shared by the kernels that must match it bit for bit: the sinc window of the warp (ccd_inter.hip) and the
// Box-Muller step of common randomness (ccd_float.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ccd {
__device__ __forceinline__ double trig_sin_core(double r) {
    const double r2 = r * r;
    double p = -7.6471637318198164759e-13;
    p = fma(p, r2, 1.6059043836821614599e-10);
    p = fma(p, r2, -2.5052108385441718775e-08);
    p = fma(p, r2, 2.7557319223985890653e-06);
    p = fma(p, r2, -1.9841269841269841270e-04);
    p = fma(p, r2, 8.3333333333333333333e-03);
    p = fma(p, r2, -1.6666666666666666667e-01);
    return fma(p * r2, r, r);
}
__device__ __forceinline__ double trig_cos_core(double r) {
    const double r2 = r * r;
    double p = 4.7794773323873852974e-14;
    p = fma(p, r2, -1.1470745597729724714e-11);
    p = fma(p, r2, 2.0876756987868098979e-09);
    p = fma(p, r2, -2.7557319223985890653e-07);
    p = fma(p, r2, 2.4801587301587301587e-05);
    p = fma(p, r2, -1.3888888888888888889e-03);
    p = fma(p, r2, 4.1666666666666666667e-02);
    p = fma(p, r2, -0.5);
    return fma(p, r2, 1.0);
}
// x = q * pi / 2 + r: returns r in [-pi / 4, pi / 4] and the quadrant q & 3
__device__ __forceinline__ double trig_reduce(double x, int* quadrant) {
    const double q = rint(x * 6.36619772367581382433e-01);
    double r = fma(-q, 1.57079632679489655800e+00, x);
    r = fma(-q, 6.12323399573676603587e-17, r);
    *quadrant = static_cast<int>(q) & 3;
    return r;
}
}  // namespace ccd
