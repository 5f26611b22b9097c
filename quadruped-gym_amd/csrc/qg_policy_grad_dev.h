// qg_policy_grad_dev.h -- the device routines the two backward passes of the fused MLP policy share (qg_policy_grad.hip: the PPO loss;
// qg_policy_distill.hip: the imitation loss): the product over an operand image and the sum over a tile's rows.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include "qg_policy.h"

#define QGG_WAVES 4

// sum += (operand image block row m, nk blocks of 16 along k) . (activations in the register image).  A block of 16 is one f32 chain of
// the matrix instruction (16 exact products, as the forward pass); the blocks are added in f64 -- the pass differentiates sums with heavy
// cancellation over the rows, and a pre-activation that is good to the last f32 bit keeps its error at that of torch's blocked sums.
// Operands come in groups of four blocks, the next group's loads issued before this group's matrix instructions (indices past the end
// are clamped and the instructions guarded, wave-uniformly): a wave waits for memory once per group, not once per block.
__device__ __forceinline__ void qgg_load_group(qgp_f32x4 (&a)[4], qgp_f32x4 (&b)[4], const qgp_f32x4 *w, const qgp_f32x4 *xin, int q0, int nk, int lane) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int q = min(q0 + u, nk - 1);
        a[u] = w[q * 64];
        b[u] = xin[q * 64 + lane];
    }
}

__device__ __forceinline__ void qgg_product(const float *__restrict__ image, int nk, int m, const qgp_f32x4 *xin, double (&sum)[4], int lane) {
    const qgp_f32x4 *w = (const qgp_f32x4 *)image + (size_t)m * nk * 64 + lane;
    qgp_f32x4 a[4], b[4], an[4], bn[4];
    qgg_load_group(a, b, w, xin, 0, nk, lane);
    for (int q0 = 0; q0 < nk; q0 += 4) {
        qgg_load_group(an, bn, w, xin, q0 + 4, nk, lane);
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (q0 + u < nk) {
                qgp_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 4; s++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][s], b[u][s], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; r++) sum[r] += (double)acc[r];
            }
#pragma unroll
        for (int u = 0; u < 4; u++) a[u] = an[u], b[u] = bn[u];
    }
}

// the sum over the 16 rows of a tile (lanes that differ in their low four bits): a fixed butterfly, the same value in every lane
__device__ __forceinline__ double qgg_sum_rows(double v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

// the weight-gradient launch of qg_policy_grad.hip over the work items of `g` (a copy of the handle's KGrad whose n_items ends after
// the actor's items launches the actor's alone: the item after them then adds the tiles' scalars)
int qg_policy_grad_launch_weights(qg_policy *p, const KGrad &g, int tiles, int slots, hipStream_t st);
