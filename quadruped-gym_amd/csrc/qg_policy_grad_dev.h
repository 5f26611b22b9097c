// qg_policy_grad_dev.h -- what the two backward passes of the fused MLP policy share (qg_policy_grad.hip: the PPO loss;
// qg_policy_distill.hip: the imitation loss): the product over an operand image, the two sums over a tile's rows, the shell of a rows
// kernel around its heads, and the host side's geometry and row checks.  Internal.
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

// The sum over the 16 rows of a tile (lanes that differ in their low four bits), the same value in every lane -- twice, on purpose, and
// not to be merged: the two group the additions differently, so the last bit of a sum depends on which one formed it.
// A fixed butterfly: four steps.  The PPO heads take it: their guarantee is the same bits for the same batch, which any fixed grouping gives.
__device__ __forceinline__ double qgg_sum_rows(double v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

// Ascending row order: sixteen steps.  The distillation heads take it: rows that add zero are then no-ops whatever their place in the tile,
// which the placement guarantee of the pass needs (live rows among rows of weight zero give the same bits wherever they sit; in the
// butterfly a zero row changes which partial sums meet).
__device__ __forceinline__ double qgd_sum_rows(double v, int lane) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 16; j++) s += __shfl(v, (lane & 48) | j);
    return s;
}

// ---- the shell of a rows kernel ----------------------------------------------------------------------------------------------------------
// A rows kernel -- a workgroup of QGG_WAVES waves per tile of 16 rows -- is shell, heads, shell: stage the observation tile, run the layers
// forward with every layer's input and tanh' stored in the row records, form the heads of its loss on wave 0, walk back over the
// transposed image.  The shell is the text below, ONCE; a kernel keeps the loop skeleton and its own heads (qg_policy_grad_rows_kernel
// shows the order).  Statement macros, not device functions: DESIGN.md, "Shared kernel text" -- the function forms tried on these two
// kernels moved the argument loads and the register assignment from the first instructions on (docs/EXPERIMENTS.md).  After an edit
// here: `make asm` before and after, then tools/asm_diff.py.  The text is pasted, not evaluated; besides its arguments it reads the names
// every rows kernel has: the parameters P, G, packed, packed_t, n, rec, and what QGG_ROWS_ENTRY declares.

// Declares tower (TOWER: blockIdx.y, or a constant), tile, row0, lane, e, g, wave, the two activation buffers x0 / x1, myrec, and
// in_width, the padded width of the tower's input.
#define QGG_ROWS_ENTRY(TOWER)                                                                                                              \
    extern __shared__ qgp_f32x4 qgg_lds[];                                                                                                 \
    const int tower = TOWER, tile = blockIdx.x, row0 = tile * QGP_TILE;                                                                    \
    const int lane = threadIdx.x & 63, e = lane & 15, g = lane >> 4;                                                                       \
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                                                                     \
    float *x0 = (float *)qgg_lds;                                                                                                          \
    float *x1 = x0 + P.lds0_floats;                                                                                                        \
    float *myrec = rec + (size_t)(row0 + e) * G.rec; /* the record of this lane's row (rows past n in the last tile have one too) */       \
    const int in_width = 16 * P.layer[tower][0].nq

// Stages the tower's window of the observation tile -- columns [IN_OFF, IN_OFF + IN_DIM) of the rows of OBS, OBS_STRIDE apart --, zero
// padded, into buffer 0 in the operand image (as the forward pass) and into the records; declares nl.
#define QGG_ROWS_STAGE(IN_DIM, IN_OFF, OBS, OBS_STRIDE)                                                                                    \
    for (int idx = threadIdx.x; idx < QGP_TILE * in_width; idx += 64 * QGG_WAVES) {                                                        \
        const int ee = idx / in_width, c = idx - ee * in_width;                                                                            \
        float v = 0.f;                                                                                                                     \
        if (c < IN_DIM && row0 + ee < n) v = OBS[(size_t)(row0 + ee) * OBS_STRIDE + IN_OFF + c];                                           \
        x0[((c >> 2) * 16 + ee) * 4 + (c & 3)] = v;                                                                                        \
        rec[(size_t)(row0 + ee) * G.rec + G.layer[tower][0].h_off + c] = v;                                                                \
    }                                                                                                                                      \
    const int nl = P.n_layers

// Layer l of the forward loop: declares L, xin, xout; the barrier says the layer's input is complete (and the buffer it overwrites has been
// read by every wave).
#define QGG_ROWS_LAYER(l)                                                                                                                  \
    const KPolLayer L = P.layer[tower][l];                                                                                                 \
    const qgp_f32x4 *xin = (const qgp_f32x4 *)((l & 1) ? x1 : x0);                                                                         \
    qgp_f32x4 *xout = (qgp_f32x4 *)((l & 1) ? x0 : x1);                                                                                    \
    __syncthreads()

// A hidden layer: its blocks over the waves; h to the other buffer and to the record as the next layer's input, tanh' kept where this
// thread will put the block's delta.
#define QGG_ROWS_HIDDEN(l)                                                                                                                 \
    {                                                                                                                                      \
        const int h_next = G.layer[tower][l + 1].h_off, d_own = G.layer[tower][l].d_off;                                                   \
        for (int m = wave; m < L.nb; m += QGG_WAVES) {                                                                                     \
            const qgp_f32x4 bias = *(const qgp_f32x4 *)(packed + L.b_off + 16 * m + 4 * g);                                                \
            double sum[4] = {(double)bias[0], (double)bias[1], (double)bias[2], (double)bias[3]};                                          \
            qgg_product(packed + L.w_off, L.nq, m, xin, sum, lane);                                                                        \
            qgp_f32x4 h, dh;                                                                                                               \
            _Pragma("unroll") for (int r = 0; r < 4; r++) { /* tanh and its derivative in f64, each rounded once */                        \
                const double t = tanh(sum[r]);                                                                                             \
                h[r] = (float)t;                                                                                                           \
                dh[r] = (float)(1.0 - t * t);                                                                                              \
            }                                                                                                                              \
            xout[m * 64 + lane] = h;                                                                                                       \
            *(qgp_f32x4 *)(myrec + h_next + 16 * m + 4 * g) = h;                                                                           \
            *(qgp_f32x4 *)(myrec + d_own + 16 * m + 4 * g) = dh;                                                                           \
        }                                                                                                                                  \
    }

// The output layer (wave 0): declares acc[4], the pre-activations of this lane's four outputs of row e (f64), and row, live.
#define QGG_ROWS_OUTPUT(l)                                                                                                                 \
    const qgp_f32x4 bias = *(const qgp_f32x4 *)(packed + L.b_off + 4 * g);                                                                 \
    double acc[4] = {(double)bias[0], (double)bias[1], (double)bias[2], (double)bias[3]};                                                  \
    qgg_product(packed + L.w_off, L.nq, 0, xin, acc, lane);                                                                                \
    const int row = row0 + e;                                                                                                              \
    const bool live = row < n

// ... and its delta D, from the heads, to the other buffer and to the record
#define QGG_ROWS_DELTA(l, D)                                                                                                               \
    xout[lane] = D;                                                                                                                        \
    *(qgp_f32x4 *)(myrec + G.layer[tower][l].d_off + 4 * g) = D

// Back through the layers: delta_l sits in the buffer layer l wrote its output to; delta_{l-1} = (W_l^T delta_l) tanh' goes to the other,
// and into the record over the tanh' this thread stored there on the way forward.
#define QGG_ROWS_WALK_BACK()                                                                                                               \
    for (int l = nl - 1; l >= 1; l--) {                                                                                                    \
        const KPolLayer L = P.layer[tower][l];                                                                                             \
        const KGradLayer GL = G.layer[tower][l];                                                                                           \
        const int d_prev = G.layer[tower][l - 1].d_off;                                                                                    \
        const qgp_f32x4 *din = (const qgp_f32x4 *)((l & 1) ? x0 : x1);                                                                     \
        qgp_f32x4 *dout = (qgp_f32x4 *)((l & 1) ? x1 : x0);                                                                                \
        __syncthreads();                                                                                                                   \
        for (int m = wave; m < L.nq; m += QGG_WAVES) { /* the blocks of layer l's input = of layer l - 1's output */                       \
            double sum[4] = {0.0, 0.0, 0.0, 0.0};                                                                                          \
            qgg_product(packed_t + GL.wt_off, L.nb, m, din, sum, lane); /* W^T delta */                                                    \
            const qgp_f32x4 dh = *(const qgp_f32x4 *)(myrec + d_prev + 16 * m + 4 * g);                                                    \
            qgp_f32x4 d;                                                                                                                   \
            _Pragma("unroll") for (int r = 0; r < 4; r++) d[r] = (float)(sum[r] * (double)dh[r]);                                          \
            dout[m * 64 + lane] = d;                                                                                                       \
            *(qgp_f32x4 *)(myrec + d_prev + 16 * m + 4 * g) = d;                                                                           \
        }                                                                                                                                  \
    }

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// the partition of a pass over B rows (a function of B alone) and the rows kernel's LDS bytes
struct QgGradGeom {
    int tiles, slots;
    size_t lds;
};
QgGradGeom qg_policy_grad_geom(const qg_policy *p, int32_t B);

// what both entry points ask of the rows: 1 <= B <= the rows reserved, and a row stride that holds the actor's window -- and the critic's
// where the critic is launched.  `who` is the entry point's name, for the message.
int qg_policy_grad_check_rows(const qg_policy *p, const char *who, int32_t B, int32_t obs_stride, bool with_critic);

// the weight-gradient launch of qg_policy_grad.hip over the work items of `g` (a copy of the handle's KGrad whose n_items ends after
// the actor's items launches the actor's alone: the item after them then adds the tiles' scalars)
int qg_policy_grad_launch_weights(qg_policy *p, const KGrad &g, int tiles, int slots, hipStream_t st);
