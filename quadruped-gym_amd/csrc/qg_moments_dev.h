// qg_moments_dev.h -- the f64 moments the running normaliser (qg_norm.hip) and the reward monitor (qg_monitor.hip) both keep: a
// (count, mean, M2) triple per run of values, M2 = sum (x - mean)^2.  Internal: not installed; device code only.
//
// Numerics.  A thread accumulates sum(x - K) and sum((x - K)^2) in f64 with K its first value: x - K is exact in f64 for f32 inputs,
// so a constant run gives M2 = 0 exactly.  qg_moments_finish turns the shifted sums into (mean, M2); everything above a thread is
// Chan's pairwise merge, qg_moments_merge.  Never E[x^2] - E[x]^2.  The order of the merges is the caller's and part of its bits: a
// fixed function of the shape, never of the timing (no atomics).
#pragma once
#include <hip/hip_runtime.h>

// (na, ma, Ma) <- merge with (nb, mb, Mb): Chan et al.  Either side may be empty.
__device__ __forceinline__ void qg_moments_merge(double &na, double &ma, double &Ma, double nb, double mb, double Mb) {
    if (nb == 0.0) return;
    if (na == 0.0) {
        na = nb, ma = mb, Ma = Mb;
        return;
    }
    const double n = na + nb, d = mb - ma, f = nb / n;
    ma = ma + d * f;
    Ma = Ma + Mb + d * d * na * f;
    na = n;
}

// shifted sums -> (mean, M2)
__device__ __forceinline__ void qg_moments_finish(double cnt, double K, double s1, double s2, double &mean, double &M2) {
    if (cnt == 0.0) {
        mean = 0.0, M2 = 0.0;
        return;
    }
    mean = K + s1 / cnt;
    M2 = fmax(s2 - s1 * s1 / cnt, 0.0);
}

// Chan's merge over the 64 lanes: lane l takes lane l ^ off as the right-hand side where l < l ^ off, and is the right-hand side
// otherwise -- both lanes of a pair compute merge(lower, upper), so every lane ends with the same bits
__device__ __forceinline__ void qg_moments_wave_merge(int lane, double &cnt, double &mean, double &M2) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double oc = __shfl_xor(cnt, off, 64), om = __shfl_xor(mean, off, 64), oM = __shfl_xor(M2, off, 64);
        if (lane & off) {
            double a = oc, b = om, c = oM;
            qg_moments_merge(a, b, c, cnt, mean, M2);
            cnt = a, mean = b, M2 = c;
        } else {
            qg_moments_merge(cnt, mean, M2, oc, om, oM);
        }
    }
}
