// What the kernels on the CTC lattice (k_ctc, k_ctc_fast of qk_ctc.hip, k_ctc_align of qk_ctc_align.hip) share: the "no path" value
// and its threshold, the log-sum-exp of the recursions, the geometry they are launched with, and lp = u - lse.  Only what is the SAME
// code in every user AND compiles to the same instructions as the copy it replaces lives here.  The per-sample clamps, the per-thread
// state (lab_s, cls, the skips), the table u = log(p + eps) and the frame normaliser did not pass the second test and stay written
// out in each kernel ("what the CTC family shares").  The transducer lattice (qk_rnnt.hip) is a different one, and the
// log1pf log-add-exps of qk_ctc_decode.hip and qk_rnnt.hip are different arithmetic: neither shares anything with this.
#pragma once

#include "qk_common.h"

namespace qk {

constexpr float kNegInf = -1e30f;          // log 0 of the lattice: finite, so that sums of two stay finite
constexpr float kDead = -1e29f;            // at or below: no path reaches the cell

__device__ __forceinline__ float lse2(float a, float b)
{
    const float m = fmaxf(a, b);
    if (m <= kDead) return kNegInf;
    return m + __logf(__expf(a - m) + __expf(b - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c)
{
    const float m = fmaxf(a, fmaxf(b, c));
    if (m <= kDead) return kNegInf;
    return m + __logf(__expf(a - m) + __expf(b - m) + __expf(c - m));
}

// B samples of T frames and C classes (blank = C - 1), Lmax label slots, Smax = 2 Lmax + 1 states; u = log(p + eps)
struct LatticeGeom { int B, T, C, Lmax, Smax; float eps; };

// lp[t][c] = u[t][c] - lse[t] over the first n = Tn C elements of the table in LDS, in place, by THREADS threads
template <int THREADS>
__device__ __forceinline__ void lattice_normalise(float *lpt, const float *lse, int n, int C, int tid)
{
    for (int e = tid; e < n; e += THREADS) lpt[e] -= lse[e / C];
}

}  // namespace qk
