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

// (qgg_product, qgd_sum_rows and the QGG_ROWS_* shell of a rows kernel: qg_policy_grad_dev.h)

__global__ __launch_bounds__(64 * QGG_WAVES) void qg_policy_distill_rows_kernel(KPolicy P, KGrad G, qg_distill_params dp, const float *__restrict__ packed,
                                                                               const float *__restrict__ packed_t, int n, qg_distill_batch bt,
                                                                               float *rec, double *__restrict__ tile_misc) {
    QGG_ROWS_ENTRY(0);          // the actor's tower alone, and its window of the row
    QGG_ROWS_STAGE(P.obs_dim, 0, bt.obs, bt.obs_stride);
    for (int l = 0; l < nl; l++) {
        QGG_ROWS_LAYER(l);
        if (l < nl - 1) {
            QGG_ROWS_HIDDEN(l);
            continue;
        }
        if (wave != 0) continue;
        // ---- the heads of the tile's rows (f64), and the output layer's delta ----
        QGG_ROWS_OUTPUT(l);
        const bool kl = dp.loss == QG_DISTILL_KL;
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
        QGG_ROWS_DELTA(l, d);
    }
    QGG_ROWS_WALK_BACK();
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
    // (params and batch are refused before the handle is looked at, so B < 1 is refused here; qg_policy_grad_check_rows needs the handle)
    if (B < 1) return fail(QG_ERR_ARG, "qg_policy_distill_grad_device: B must be >= 1");
    if (!bt->obs || !bt->target_mean) return fail(QG_ERR_ARG, "qg_distill_batch: null obs or target_mean");
    if (dp->loss == QG_DISTILL_KL && !bt->target_log_std) return fail(QG_ERR_ARG, "qg_distill_batch: QG_DISTILL_KL needs target_log_std");
    if (!p) return fail(QG_ERR_ARG, "qg_policy_distill_grad_device: null policy");
    QG_TRY(qg_policy_grad_check_rows(p, "qg_policy_distill_grad_device", B, bt->obs_stride, false));
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    const hipStream_t st = (hipStream_t)stream;
    const QgGradGeom geo = qg_policy_grad_geom(p, B);
    qg_policy_distill_rows_kernel<<<dim3((unsigned)geo.tiles, 1u), 64 * QGG_WAVES, geo.lds, st>>>(p->k, p->g, *dp, p->d_packed, p->d_packed_t, B, *bt,
                                                                                             p->d_rec, p->d_tile_misc);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    // the actor's work items alone: the weights kernel takes the item after the last as the one that adds the tiles' scalars, and an
    // item below the critic's first never selects a critic layer
    KGrad actor = p->g;
    if (p->k.n_towers == 2) actor.n_items = p->g.layer[1][0].item0 + 1;
    QG_TRY(qg_policy_grad_launch_weights(p, actor, geo.tiles, geo.slots, st));
    const int threads = 256;
    qg_policy_distill_reduce_kernel<<<(p->n_params + threads - 1) / threads + 1, threads, 0, st>>>(
        p->k, *dp, B, geo.tiles, geo.slots, p->n_params, p->d_partial, p->d_slot_misc, p->d_tile_misc, grad, stats);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}
