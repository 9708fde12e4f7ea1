// ccd_laplace.hpp - the leaky quantised Laplace model's left cumulative (constriction 0.4.2 QuantizedLaplace(-64, 63),
// 24-bit precision) as BOTH entropy kernels evaluate it: f64 exp the way glibc does it + the host's RN(1 / b) table.  What must
// agree with the encoder's libm is the 24-bit integer boundary, and that is proven on the whole reachable domain (32 768 mu
// indices x 2 561 scale indices x 127 symbols = 1.0658e10 boundaries: tools/cdf_sweep.py, profiles/r03/cdf_sweep.log;
// tests/test_gpu_parity.py::test_laplace_boundaries_sweep keeps every 64th scale index in the GPU suite).
#pragma once

#include "ccd_device.hpp"

namespace ccd {

// exp(x) / 2 for x <= 0 in f64, the way glibc does it: x = (128 k' + j) ln2 / 128 + r with |r| <= ln2 / 256, e^x = 2^k' * T[j] *
// (1 + r + r^2/2 + .. + r^5/120) with T[j] = 2^(j/128) from a 1 KB table (LDS in the kernel), two-part ln2 / 128.  13 f64
// operations and a Horner chain of depth 4 instead of 21 and depth 7 for the table-free degree-13 version it replaced.  Error
// ~1 ulp; what matters is floor(16777088 * cdf), and THAT is proven on the whole reachable domain: tools/cdf_sweep.py compares all 1.0658e10 boundaries with libm (profiles/r03/cdf_sweep.log).
#ifndef CCD_EXP_LOG
#define CCD_EXP_LOG 7
#endif
#ifndef CCD_EXP_DEG
#define CCD_EXP_DEG 5
#endif
#ifndef CCD_EXP_INC
#define CCD_EXP_INC "ccd_exp_table.inc"
#endif
static __device__ const double kExpTab[1 << CCD_EXP_LOG] = {  // (one copy per translation unit: the two kernels do not link device code)
#include CCD_EXP_INC
};
constexpr int kExpLog = CCD_EXP_LOG, kExpN = 1 << kExpLog;
__device__ __forceinline__ double exp_nonpos(double x, const double* tab /* 2^(j/N): LDS in the kernel */) {
    // No clamp for very negative x: kd stays finite, 2^(ki >> log N) underflows to an exact 0 in v_ldexp_f64 (and 1 - 0 == 1), which
    // is what the 24-bit cumulative needs; |x| <= 128 / min scale = 1.9e4 here, far from where ki could overflow.
    const double kd = rint(x * ldexp(0x1.71547652b82fep+0, kExpLog));            // N / ln 2
    double r = fma(kd, -ldexp(0x1.62e42fef00000p-1, -kExpLog), x);               // ln 2 / N, leading 33 bits: kd * hi is exact below 2^20
    r = fma(kd, -ldexp(0x1.473de6af278edp-34, -kExpLog), r);
    const int ki = static_cast<int>(kd);
    const double t = tab[ki & (kExpN - 1)];
    const double r2 = r * r;
#if CCD_EXP_DEG == 5
    double p = fma(r, 8.333333333333333e-03, 4.1666666666666664e-02);  // 1/5!, 1/4!
    p = fma(p, r, 1.6666666666666666e-01);
    p = fma(p, r, 0.5);
#elif CCD_EXP_DEG == 4
    double p = fma(r, 4.1666666666666664e-02, 1.6666666666666666e-01);
    p = fma(p, r, 0.5);
#elif CCD_EXP_DEG == 3
    double p = fma(r, 1.6666666666666666e-01, 0.5);
#else
    double p = 0.5;
#endif
    p = fma(p, r2, r);                                            // e^r - 1
    return ldexp(fma(t, p, t), (ki >> kExpLog) - 1);              // e^x / 2 (the caller's 0.5 *, folded into the exponent)
}

// Left cumulative of symbol s under (mu, b) with rcp = RN(1 / b) from the host.  The quotient (x - mu) / b is formed as
// (x - mu) * rcp WITHOUT the Newton step that would make it the correctly rounded quotient: with or without it, with or
// without a clamp of very negative arguments, all 1.0658e10 reachable boundaries equal libm's (tools/cdf_sweep.py) - the
// proof is the enumeration, not the error analysis.
__device__ __forceinline__ uint32_t window_left(double mu, double rcp, int s, const double* exp_tab) {
    const double x = static_cast<double>(s) - 0.5;
    const double d = x - mu;
    const double e = exp_nonpos(-fabs(d) * rcp, exp_tab);  // e^(-|x - mu| / b) / 2
    const double cdf = d <= 0.0 ? e : 1.0 - e;
    const uint32_t v = static_cast<uint32_t>(16777088.0 * cdf) + static_cast<uint32_t>(s - kAcLo);
    return s <= kAcLo ? 0u : (s > kAcLo + kAlphabet - 1 ? (1u << kRcPrecision) : v);
}

// The same boundary from integers, for the production kernel's table builder (the producers' late path pays per issued
// instruction).  mu = -64 + mu_idx / 256 and x = s - 0.5, so d = x - mu = (256 s + 16256 - mu_idx) / 256: window_left forms mu,
// x and d in f64 without a single rounding (every one a multiple of 2^-8 below 2^8), this forms 256 d with one integer
// subtraction.  With rcp256 = rcp * 2^-8 (exact: rcp >= RN(1 / b_max) is nowhere near the subnormals) the product
// |256 d| * rcp256 is RN of the same real number as |d| * rcp: same bits, and everything behind it is window_left's.
__device__ __forceinline__ int window_d256(int mu_idx, int s) { return 256 * s + (256 * 64 - 128) - mu_idx; }
__device__ __forceinline__ double window_rcp256(double rcp) { return ldexp(rcp, -8); }
// floor(16777088 cdf) alone: a caller that knows where its symbols lie applies window_left's edge cases (s <= -64, s > 63) itself
__device__ __forceinline__ uint32_t window_cum_d256(int d256, double rcp256, const double* exp_tab) {
    const double e = exp_nonpos(-fabs(static_cast<double>(d256)) * rcp256, exp_tab);  // e^(-|x - mu| / b) / 2
    const double cdf = d256 <= 0 ? e : 1.0 - e;
    return static_cast<uint32_t>(16777088.0 * cdf);
}
__device__ __forceinline__ uint32_t window_left_d256(int d256, double rcp256, int s, const double* exp_tab) {
    const uint32_t v = window_cum_d256(d256, rcp256, exp_tab) + static_cast<uint32_t>(s - kAcLo);
    return s <= kAcLo ? 0u : (s > kAcLo + kAlphabet - 1 ? (1u << kRcPrecision) : v);
}

}  // namespace ccd
