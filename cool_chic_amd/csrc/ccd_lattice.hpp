// ccd_lattice.hpp - the geometry of the probe lattices of the distortion deltas, stated once for the
// planner (ccd_dsens_api.cpp) and for dsens_dep_kernel (ccd_inter.hip).  All of it is __host__ __device__;
// ccd_debug_lattice_stride and ccd_debug_lattice_hit (ccd_dsens_api.cpp) run it on the host for tests/test_dependent_deltas.py.
//
// One axis of a grid: n latents over N samples.  A move of latent i can change the decoded samples of its clipped footprint
// interval [max(s(i) + lo, 0), min(s(i) + hi, N - 1)], s(i) = floor(i num / den) (ccd_latent_footprint).  Read as a REFERENCE of
// another frame the planes go through planes_to_444_kernel first, which repeats 4:2:0 chroma 2 x 2: the region that changes there
// is the interval widened outwards to even alignment, [a & ~1, b | 1] (`even`).  That is the reference-change region E(i).  Both
// ends of E(i) do not decrease with i.
// Only DIRECT readers of the reference are described: what a frame that predicts from a dependent reads is not followed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ccd {

struct LatticeAxis {
    int32_t n, N;        // latents, samples
    int32_t lo, hi;      // the footprint interval around s(i)
    uint32_t num, den;   // s(i) = floor(i num / den)
    int32_t even;        // widen to even alignment (4:2:0)
};

__host__ __device__ inline void lattice_region(const LatticeAxis& A, int i, int& a, int& b) {
    const int64_t s = static_cast<int64_t>(static_cast<uint64_t>(i) * A.num / A.den);
    const int64_t lo = s + A.lo, hi = s + A.hi;
    a = static_cast<int>(lo < 0 ? 0 : lo);
    b = static_cast<int>(hi > A.N - 1 ? A.N - 1 : hi);
    if (A.even) { a &= ~1; b |= 1; }
}

// The smallest S such that at least `margin` samples lie strictly between E(i) and E(i + S) for every i; n (at least 1) when
// no stride below n does.  margin 0: the regions of two lattice neighbours are disjoint, the stride of the own maps.
__host__ __device__ inline int lattice_stride(const LatticeAxis& A, int margin) {
    for (int S = 1; S < A.n; ++S) {
        bool ok = true;
        for (int i = 0; ok && i + S < A.n; ++i) {
            int a0, b0, a1, b1;
            lattice_region(A, i, a0, b0);
            lattice_region(A, i + S, a1, b1);
            ok = static_cast<int64_t>(a1) - b0 - 1 >= margin;
        }
        if (ok) return S;
    }
    return A.n > 1 ? A.n : 1;
}

// The members i = phase + k S (i < n) of a lattice whose E(i) intersects the sample interval [a, b]: returns how many, and the
// first of them in *first (they are consecutive members: the ends of E do not decrease).  One bisection for the first member
// whose region ends at or behind a, then a walk while regions begin at or before b.
__host__ __device__ inline int lattice_hit(const LatticeAxis& A, int S, int phase, int a, int b, int* first) {
    *first = -1;
    if (phase >= A.n || a > b) return 0;
    const int nk = (A.n - 1 - phase) / S + 1;
    int lo = 0, hi = nk;  // the first k in [0, nk] with E(k).b >= a (nk: none)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int ea, eb;
        lattice_region(A, phase + mid * S, ea, eb);
        if (eb >= a) hi = mid; else lo = mid + 1;
    }
    int count = 0;
    for (int k = lo; k < nk; ++k) {
        int ea, eb;
        lattice_region(A, phase + k * S, ea, eb);
        if (ea > b) break;  // (no region is empty: lo <= 0 <= hi and 0 <= s(i) < N)
        if (count == 0) *first = phase + k * S;
        ++count;
    }
    return count;
}

}  // namespace ccd
