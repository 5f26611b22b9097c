// qg_policy_distill.hip -- the imitation loss of teacher-student distillation and its gradient for the fused MLP policy
// (include/quadgym.h: qg_policy_distill_grad_device).  DESIGN 4.19.
//
// The three-stage pass of qg_policy_grad.hip on the actor's tower alone, in the scratch of qg_policy_reserve_grad:
//   1. rows    -- qg_policy_distill_rows_kernel, a workgroup (four waves) per tile of 16 rows: the forward pass recomputed in the forward
//                 kernel's register image, the heads of the tile's rows in f64 on wave 0 (the squared error or the KL divergence against
//                 the target means, weighted per row), the walk back over the transposed operand image.  Every layer's h and delta go
//                 into the row records, the tile's scalar sums (log_std terms, loss, squared error, weight) and its largest |mu - t|
//                 into tile_misc.
//   2. weights -- qg_policy_grad_weights_kernel as it is, over the actor's work items: the item after them adds the tiles' scalars.
//   3. reduce  -- qg_policy_distill_reduce_kernel: a thread per parameter adds the slots in ascending order (f64, rounded once); the
//                 critic's entries, and log_std in MSE mode, are written as +0.0; one more workgroup takes the maximum over the tiles and
//                 writes stats.
// No atomics, no workgroup waits for another, the partition is a function of B alone.  A row of weight zero has zero deltas: it puts
// exact zeros into every chain.

#include <hip/hip_runtime.h>

#include <cmath>

#include "qg_policy_grad_dev.h"

#define QGD_MISC_LOSS 16          // tile_misc / slot_misc: sum_rows w l, sum_rows w sum_a (mu - t)^2, sum_rows w (behind the 16 log_std terms)
#define QGD_MISC_SQ 17
#define QGD_MISC_W 18
#define QGD_MISC_MAX 20           // tile_misc alone (the weights launch does not add the entries past 19): max |mu - t| of the tile

// the sum over the 16 rows of a tile in ascending row order, the same value in every lane: rows that add zero are then no-ops, whatever
// their place in the tile
__device__ __forceinline__ double qgd_sum_rows(double v, int lane) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 16; j++) s += __shfl(v, (lane & 48) | j);
    return s;
}

__global__ __launch_bounds__(64 * QGG_WAVES) void qg_policy_distill_rows_kernel(KPolicy P, KGrad G, qg_distill_params dp, const float *__restrict__ packed,
                                                                               const float *__restrict__ packed_t, int n, qg_distill_batch bt,
                                                                               float *rec, double *__restrict__ tile_misc) {
    extern __shared__ qgp_f32x4 qgd_lds[];
    const int tile = blockIdx.x, row0 = tile * QGP_TILE;
    const int lane = threadIdx.x & 63, e = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *x0 = (float *)qgd_lds;
    float *x1 = x0 + P.lds0_floats;
    float *myrec = rec + (size_t)(row0 + e) * G.rec;          // the record of this lane's row (rows past n in the last tile have one too)

    // the actor's window of the observation tile, zero padded, into buffer 0 in the operand image and into the records
    {
        const int width = 16 * P.layer[0][0].nq;
        for (int idx = threadIdx.x; idx < QGP_TILE * width; idx += 64 * QGG_WAVES) {
            const int ee = idx / width, c = idx - ee * width;
            float v = 0.f;
            if (c < P.obs_dim && row0 + ee < n) v = bt.obs[(size_t)(row0 + ee) * bt.obs_stride + c];
            x0[((c >> 2) * 16 + ee) * 4 + (c & 3)] = v;
            rec[(size_t)(row0 + ee) * G.rec + G.layer[0][0].h_off + c] = v;
        }
    }

    const int nl = P.n_layers;
    for (int l = 0; l < nl; l++) {
        const KPolLayer L = P.layer[0][l];
        const qgp_f32x4 *xin = (const qgp_f32x4 *)((l & 1) ? x1 : x0);
        qgp_f32x4 *xout = (qgp_f32x4 *)((l & 1) ? x0 : x1);
        __syncthreads();          // the layer's input is complete (and the buffer it overwrites has been read by every wave)
        if (l < nl - 1) {
            const int h_next = G.layer[0][l + 1].h_off, d_own = G.layer[0][l].d_off;
            for (int m = wave; m < L.nb; m += QGG_WAVES) {
                const qgp_f32x4 bias = *(const qgp_f32x4 *)(packed + L.b_off + 16 * m + 4 * g);
                double sum[4] = {(double)bias[0], (double)bias[1], (double)bias[2], (double)bias[3]};
                qgg_product(packed + L.w_off, L.nq, m, xin, sum, lane);
                qgp_f32x4 h, dh;
#pragma unroll
                for (int r = 0; r < 4; r++) {            // tanh and its derivative in f64, each rounded once
                    const double t = tanh(sum[r]);
                    h[r] = (float)t;
                    dh[r] = (float)(1.0 - t * t);
                }
                xout[m * 64 + lane] = h;
                *(qgp_f32x4 *)(myrec + h_next + 16 * m + 4 * g) = h;
                *(qgp_f32x4 *)(myrec + d_own + 16 * m + 4 * g) = dh;      // kept where this thread will put the block's delta
            }
            continue;
        }
        if (wave != 0) continue;
        // ---- the heads of the tile's rows (f64), and the output layer's delta ----
        const qgp_f32x4 bias = *(const qgp_f32x4 *)(packed + L.b_off + 4 * g);
        double acc[4] = {(double)bias[0], (double)bias[1], (double)bias[2], (double)bias[3]};
        qgg_product(packed + L.w_off, L.nq, 0, xin, acc, lane);
        const int row = row0 + e;
        const bool live = row < n, kl = dp.loss == QG_DISTILL_KL;
        const double w = live ? (bt.weights ? (double)bt.weights[row] : 1.0) : 0.0;
        const double scale = (double)dp.coef / (double)n * w;          // coef / B w_i
        const float *sd = packed + P.std_off;
        double *misc = tile_misc + (size_t)tile * QGG_MISC;
        qgp_f32x4 d = {0.f, 0.f, 0.f, 0.f};
        double li = 0.0, sq = 0.0, mx = 0.0, dls[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int a = 4 * g + r;
            dls[r] = 0.0;
            if (a < P.act_dim) {
                const double mu = P.out_tanh ? tanh(acc[r]) : acc[r];
                const double diff = live ? mu - (double)bt.target_mean[(size_t)row * P.act_dim + a] : 0.0;
                double dm;
                sq += diff * diff;
                mx = fmax(mx, fabs(diff));
                if (kl) {
                    const double ls = (double)sd[16 + a], lt = (double)bt.target_log_std[a];
                    const double inv_var = exp(-2.0 * ls), q = (exp(2.0 * lt) + diff * diff) * inv_var;
                    li += ls - lt + 0.5 * q - 0.5;
                    dm = scale * diff * inv_var;
                    dls[r] = scale * (1.0 - q);
                } else {
                    li += diff * diff;
                    dm = scale * 2.0 * diff;
                }
                if (P.out_tanh) dm *= 1.0 - mu * mu;
                d[r] = (float)dm;
            }
        }
        li += __shfl_xor(li, 16), sq += __shfl_xor(sq, 16), mx = fmax(mx, __shfl_xor(mx, 16));
        li += __shfl_xor(li, 32), sq += __shfl_xor(sq, 32), mx = fmax(mx, __shfl_xor(mx, 32));
        if (w == 0.0) mx = 0.0;
        mx = fmax(mx, __shfl_xor(mx, 1));
        mx = fmax(mx, __shfl_xor(mx, 2));
        mx = fmax(mx, __shfl_xor(mx, 4));
        mx = fmax(mx, __shfl_xor(mx, 8));
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double s = qgd_sum_rows(dls[r], lane);
            if (e == 0) misc[4 * g + r] = s;
        }
        const double s_l = qgd_sum_rows(w * li, lane), s_sq = qgd_sum_rows(w * sq, lane), s_w = qgd_sum_rows(w, lane);
        if (lane == 0) misc[QGD_MISC_LOSS] = s_l, misc[QGD_MISC_SQ] = s_sq, misc[QGD_MISC_W] = s_w, misc[QGD_MISC_MAX] = mx;
        xout[lane] = d;
        *(qgp_f32x4 *)(myrec + G.layer[0][l].d_off + 4 * g) = d;
    }

    // ---- back through the layers: delta_l sits in the buffer layer l wrote its output to; delta_{l-1} goes to the other ----
    for (int l = nl - 1; l >= 1; l--) {
        const KPolLayer L = P.layer[0][l];
        const KGradLayer GL = G.layer[0][l];
        const int d_prev = G.layer[0][l - 1].d_off;
        const qgp_f32x4 *din = (const qgp_f32x4 *)((l & 1) ? x0 : x1);
        qgp_f32x4 *dout = (qgp_f32x4 *)((l & 1) ? x1 : x0);
        __syncthreads();
        for (int m = wave; m < L.nq; m += QGG_WAVES) {          // the blocks of layer l's input = of layer l - 1's output
            double sum[4] = {0.0, 0.0, 0.0, 0.0};
            qgg_product(packed_t + GL.wt_off, L.nb, m, din, sum, lane);
            const qgp_f32x4 dh = *(const qgp_f32x4 *)(myrec + d_prev + 16 * m + 4 * g);      // this thread's own store of the forward part
            qgp_f32x4 d;
#pragma unroll
            for (int r = 0; r < 4; r++) d[r] = (float)(sum[r] * (double)dh[r]);
            dout[m * 64 + lane] = d;
            *(qgp_f32x4 *)(myrec + d_prev + 16 * m + 4 * g) = d;
        }
    }
}

// grad from the slots' partial sums; the last workgroup's first wave writes stats
__global__ __launch_bounds__(256) void qg_policy_distill_reduce_kernel(KPolicy P, qg_distill_params dp, int n, int n_tiles, int n_slots, int n_params,
                                                                      const float *__restrict__ partial, const double *__restrict__ slot_misc,
                                                                      const double *__restrict__ tile_misc, float *__restrict__ grad,
                                                                      float *__restrict__ stats) {
    const bool kl = dp.loss == QG_DISTILL_KL;
    if (blockIdx.x < gridDim.x - 1) {
        const int i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n_params) return;
        float out = 0.f;          // the critic (everything behind log_std), and log_std in MSE mode
        if (i < P.src_log_std) {
            double s = 0.0;
            for (int k = 0; k < n_slots; k++) s += (double)partial[(size_t)k * n_params + i];
            out = (float)s;
        } else if (kl && i < P.src_log_std + P.act_dim) {
            double s = 0.0;
            for (int k = 0; k < n_slots; k++) s += slot_misc[(size_t)k * QGG_MISC + (i - P.src_log_std)];
            out = (float)s;
        }
        grad[i] = out;
        return;
    }
    if (!stats || threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    double mx = 0.0;
    for (int t = lane; t < n_tiles; t += 64) mx = fmax(mx, tile_misc[(size_t)t * QGG_MISC + QGD_MISC_MAX]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (lane < 8) {
        double sum[3] = {0.0, 0.0, 0.0};          // w l, w (mu - t)^2, w
        for (int k = 0; k < n_slots; k++)
            for (int c = 0; c < 3; c++) sum[c] += slot_misc[(size_t)k * QGG_MISC + QGD_MISC_LOSS + c];
        const double b = (double)n;
        const double v[8] = {(double)dp.coef * sum[0] / b, sum[1] / b, kl ? sum[0] / b : 0.0, mx, sum[2], 0.0, 0.0, 0.0};
        stats[lane] = (float)v[lane];
    }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
extern "C" int qg_policy_distill_grad_device(qg_policy *p, const qg_distill_params *dp, int32_t B, const qg_distill_batch *bt, float *grad,
                                             float *stats, void *stream) {
    if (!dp || !bt || !grad) return fail(QG_ERR_ARG, "qg_policy_distill_grad_device: null params, batch or grad");
    QG_CHECK_STRUCT(dp, qg_distill_params);
    QG_CHECK_STRUCT(bt, qg_distill_batch);
    if (dp->reserved != 0) return fail(QG_ERR_ARG, "qg_distill_params.reserved must be 0");
    if (dp->loss != QG_DISTILL_MSE && dp->loss != QG_DISTILL_KL)
        return fail(QG_ERR_ARG, "qg_distill_params.loss is %d: QG_DISTILL_MSE (0) or QG_DISTILL_KL (1)", dp->loss);
    if (!qg_finite32(dp->coef)) return fail(QG_ERR_ARG, "qg_distill_params.coef must be finite");
    if (B < 1) return fail(QG_ERR_ARG, "qg_policy_distill_grad_device: B must be >= 1");
    if (!bt->obs || !bt->target_mean) return fail(QG_ERR_ARG, "qg_distill_batch: null obs or target_mean");
    if (dp->loss == QG_DISTILL_KL && !bt->target_log_std) return fail(QG_ERR_ARG, "qg_distill_batch: QG_DISTILL_KL needs target_log_std");
    if (!p) return fail(QG_ERR_ARG, "qg_policy_distill_grad_device: null policy");
    if (B > p->grad_max)
        return fail(QG_ERR_ARG, "qg_policy_distill_grad_device: B = %d, but qg_policy_reserve_grad has reserved %d rows", B, p->grad_max);
    if (bt->obs_stride < p->desc.obs_dim)
        return fail(QG_ERR_ARG, "qg_policy_distill_grad_device: obs_stride %d < obs_dim %d", bt->obs_stride, p->desc.obs_dim);
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    const hipStream_t st = (hipStream_t)stream;
    const int tiles = (B + QGP_TILE - 1) / QGP_TILE, slots = (tiles + QGG_SLOT_TILES - 1) / QGG_SLOT_TILES;
    const size_t lds = (size_t)(p->k.lds0_floats + p->k.lds1_floats) * sizeof(float);
    qg_policy_distill_rows_kernel<<<dim3((unsigned)tiles, 1u), 64 * QGG_WAVES, lds, st>>>(p->k, p->g, *dp, p->d_packed, p->d_packed_t, B, *bt,
                                                                                             p->d_rec, p->d_tile_misc);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    // the actor's work items alone: the weights kernel takes the item after the last as the one that adds the tiles' scalars, and an
    // item below the critic's first never selects a critic layer
    KGrad actor = p->g;
    if (p->k.n_towers == 2) actor.n_items = p->g.layer[1][0].item0 + 1;
    QG_TRY(qg_policy_grad_launch_weights(p, actor, tiles, slots, st));
    const int threads = 256;
    qg_policy_distill_reduce_kernel<<<(p->n_params + threads - 1) / threads + 1, threads, 0, st>>>(
        p->k, *dp, B, tiles, slots, p->n_params, p->d_partial, p->d_slot_misc, p->d_tile_misc, grad, stats);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}
