// qg_policy_grad.hip -- the PPO loss and its gradient for the fused MLP policy (include/quadgym.h: qg_policy_reserve_grad,
// qg_policy_ppo_grad_device), exact f32 on the f32-input matrix instruction (v_mfma_f32_16x16x4_f32).  DESIGN 4.11.
//
// Three launches per call, none of which waits for another workgroup, and no atomics:
//   1. rows    -- a workgroup (four waves) per tile of 16 rows and tower.  It recomputes the forward pass in the forward kernel's register
//                 image (f32 products in chains of 16, the chains and tanh in f64), forms the loss heads of its rows, and walks back:
//                 delta_{l-1} = (W_l^T delta_l) (1 - h^2) is the forward product over the TRANSPOSED operand image (qg_policy_pack_t_kernel;
//                 W^T' [input block][output block][lane] float4).  Every layer's input h and delta go, row-major, into the row's record
//                 in handle-owned scratch -- [row][feature], so the tile read along its rows is the transposed operand the next launch
//                 needs -- and the tile's scalar sums (log_std terms, loss terms) into tile_misc, f64.
//   2. weights -- a wave per (block of up to 4 x 1 16x16 blocks of one dW, slot): dW = sum_rows delta h^T is a product whose k index is
//                 the batch row, 4 rows per instruction: one f32 chain per tile, the slot's QGG_SLOT_TILES consecutive tiles added in
//                 ascending order in f64 registers; db is the same product against a column of ones.  Written to partial[slot][canonical index].  The
//                 last work item adds the slot's tile_misc rows in ascending order.
//   3. reduce  -- a thread per parameter adds the slots in ascending order (f64, rounded once) and writes grad; eight more threads
//                 write stats.
// The partition (tiles of 16 rows, slots of QGG_SLOT_TILES tiles) is a function of B alone: the same inputs give the same bits.  A row
// whose heads are zero puts exact zeros into every product (x + 0 is exact), so which tile or slot holds a row changes nothing.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "qg_policy_grad_dev.h"

// canonical flat parameters -> the transposed image of the layers past the first (one thread per packed float)
__global__ void qg_policy_pack_t_kernel(KPolicy P, KGrad G, const float *__restrict__ src, float *__restrict__ packed_t) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G.packed_t_floats) return;
    for (int t = 0; t < P.n_towers; t++)
        for (int l = 1; l < P.n_layers; l++) {
            const KPolLayer L = P.layer[t][l];
            const int off = G.layer[t][l].wt_off, wn = L.nb * L.nq * 256;
            if (i >= off && i < off + wn) {
                const int j = i - off;
                const int s = j & 3, lane = (j >> 2) & 63, rest = j >> 8;
                const int mk = rest % L.nb, qo = rest / L.nb;
                const int row = 16 * mk + 4 * (lane >> 4) + s, col = 16 * qo + (lane & 15);      // W[row][col]: k index row, output col
                packed_t[i] = (row < L.out_dim && col < L.in_dim) ? src[L.src_w + row * L.in_dim + col] : 0.f;
                return;
            }
        }
}

// (qgg_product, the product over an operand image, qgg_sum_rows and the QGG_ROWS_* shell of a rows kernel: qg_policy_grad_dev.h)

__global__ __launch_bounds__(64 * QGG_WAVES) void qg_policy_grad_rows_kernel(KPolicy P, KGrad G, qg_ppo_params pp, const float *__restrict__ packed,
                                                                            const float *__restrict__ packed_t, int n, qg_ppo_batch bt,
                                                                            float *rec, double *__restrict__ tile_misc) {
    QGG_ROWS_ENTRY(blockIdx.y);
    const int in_dim = tower ? P.layer[1][0].in_dim : P.obs_dim, in_off = tower ? P.critic_off : 0;      // the tower's window of the row (wave-uniform)
    QGG_ROWS_STAGE(in_dim, in_off, bt.obs, bt.obs_stride);
    for (int l = 0; l < nl; l++) {
        QGG_ROWS_LAYER(l);
        if (l < nl - 1) {
            QGG_ROWS_HIDDEN(l);
            continue;
        }
        if (wave != 0) continue;
        // ---- the loss heads of the tile's rows (f64), and the output layer's delta ----
        QGG_ROWS_OUTPUT(l);
        const double inv_b = 1.0 / (double)n;
        double *misc = tile_misc + (size_t)tile * QGG_MISC;
        qgp_f32x4 d = {0.f, 0.f, 0.f, 0.f};
        if (tower == 0) {
            const float *sd = packed + P.std_off;
            double lp = 0.0, z[4], inv_std[4], mu[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int a = 4 * g + r;
                z[r] = 0.0, inv_std[r] = 0.0, mu[r] = 0.0;
                if (a < P.act_dim) {
                    const double ls = (double)sd[16 + a];
                    mu[r] = P.out_tanh ? tanh(acc[r]) : acc[r];
                    inv_std[r] = exp(-ls);
                    const double act = live ? (double)bt.actions[(size_t)row * P.act_dim + a] : mu[r];
                    z[r] = (act - mu[r]) * inv_std[r];
                    lp += -0.5 * z[r] * z[r] - ls - QGG_HALF_LOG_2PI;
                }
            }
            lp += __shfl_xor(lp, 16);
            lp += __shfl_xor(lp, 32);
            const double adv = live ? (double)bt.advantages[row] : 0.0;
            const double lr = live ? lp - (double)bt.old_log_prob[row] : 0.0;
            const double ratio = exp(lr), c = (double)pp.clip_range;
            const bool clipped = (adv > 0.0 && ratio > 1.0 + c) || (adv < 0.0 && ratio < 1.0 - c);
            const double dlogp = (clipped || !live) ? 0.0 : -(adv * ratio) * inv_b;
            const double rc = fmin(fmax(ratio, 1.0 - c), 1.0 + c);
            double pol = live ? -fmin(adv * ratio, adv * rc) : 0.0;
            double kl = live ? (ratio - 1.0) - lr : 0.0;
            double cf = (live && fabs(ratio - 1.0) > c) ? 1.0 : 0.0;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int a = 4 * g + r;
                double dm = dlogp * z[r] * inv_std[r];
                if (P.out_tanh) dm *= 1.0 - mu[r] * mu[r];
                d[r] = a < P.act_dim ? (float)dm : 0.f;
                const double dls = qgg_sum_rows(a < P.act_dim ? dlogp * (z[r] * z[r] - 1.0) : 0.0);
                if (e == 0) misc[a] = dls;
            }
            pol = qgg_sum_rows(pol), kl = qgg_sum_rows(kl), cf = qgg_sum_rows(cf);
            if (lane == 0) misc[QGG_MISC_POLICY] = pol, misc[QGG_MISC_KL] = kl, misc[QGG_MISC_CLIP] = cf;
        } else {
            double vl = 0.0, dv = 0.0;
            if (live && g == 0) {
                const double v = acc[0], ret = (double)bt.returns[row], cv = (double)pp.clip_range_vf;
                double vp = v;
                bool vclip = false;
                if (cv > 0.0) {
                    const double ov = (double)bt.old_values[row], diff = v - ov;
                    vp = ov + fmin(fmax(diff, -cv), cv);
                    vclip = fabs(diff) >= cv;
                }
                vl = (ret - vp) * (ret - vp);
                dv = vclip ? 0.0 : (double)pp.vf_coef * 2.0 * (vp - ret) * inv_b;
            }
            d[0] = (float)dv;
            vl = qgg_sum_rows(vl);
            if (lane == 0) misc[QGG_MISC_VALUE] = vl;
        }
        QGG_ROWS_DELTA(l, d);
    }
    QGG_ROWS_WALK_BACK();
}

// dW (and db, on the items of input block 0) of one slot of tiles.  Matrix instruction: A[i][k] = delta[row 4s + k][16m + i],
// B[k][j] = h[row 4s + k][16q + j], lane = 16k + i resp. 16k + j; D[4 (lane >> 4) + r][lane & 15] in register r.
__global__ __launch_bounds__(64) void qg_policy_grad_weights_kernel(KPolicy P, KGrad G, int n_tiles, int n_params, const float *__restrict__ rec,
                                                                    const double *__restrict__ tile_misc, float *__restrict__ partial,
                                                                    double *__restrict__ slot_misc) {
    const int item = blockIdx.x, slot = blockIdx.y, lane = threadIdx.x;
    const int t0 = slot * QGG_SLOT_TILES, t1 = min(t0 + QGG_SLOT_TILES, n_tiles);
    if (item == G.n_items - 1) {
        if (lane < QGG_MISC) {
            double s = 0.0;
            if (lane < QGG_MISC_VALUE || (lane == QGG_MISC_VALUE && P.n_towers == 2))
                for (int t = t0; t < t1; t++) s += tile_misc[(size_t)t * QGG_MISC + lane];
            slot_misc[(size_t)slot * QGG_MISC + lane] = s;
        }
        return;
    }
    int tower = 0, layer = 0;
    for (int t = 0; t < P.n_towers; t++)
        for (int l = 0; l < P.n_layers; l++)
            if (item >= G.layer[t][l].item0) tower = t, layer = l;
    const KPolLayer L = P.layer[tower][layer];
    const KGradLayer GL = G.layer[tower][layer];
    const int idx = item - GL.item0, q = idx % L.nq, m0 = 4 * (idx / L.nq);
    const int j = lane & 15, k = lane >> 4;
    const float *hp = rec + GL.h_off + 16 * q + j;
    const float *dp[4];
#pragma unroll
    for (int i = 0; i < 4; i++) dp[i] = rec + GL.d_off + 16 * min(m0 + i, L.nb - 1) + j;
    // a tile's 16 rows are one f32 chain of the matrix instruction; the tiles of the slot are added in f64 (a 512-term f32 chain
    // would carry about 1e-6 of relative error, several times torch's blocked sums)
    double sum[4][4], sumb[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) sum[i][r] = sumb[i][r] = 0.0;
    // the 20 operand values of a tile (4 k-steps x (h, 4 deltas)); the next tile's are loaded before this tile's instructions
    float hb[4], da[4][4], hb_n[4], da_n[4][4];
    auto load_tile = [&](int t, float (&h)[4], float (&d)[4][4]) {
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const size_t base = (size_t)(t * QGP_TILE + 4 * s + k) * G.rec;
            h[s] = hp[base];
#pragma unroll
            for (int i = 0; i < 4; i++) d[s][i] = dp[i][base];
        }
    };
    load_tile(t0, hb, da);
    for (int t = t0; t < t1; t++) {
        load_tile(min(t + 1, t1 - 1), hb_n, da_n);
        qgp_f32x4 acc[4], accb[4];
#pragma unroll
        for (int i = 0; i < 4; i++) acc[i] = accb[i] = qgp_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; s++) {
#pragma unroll
            for (int i = 0; i < 4; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(da[s][i], hb[s], acc[i], 0, 0, 0);
            if (q == 0) {
#pragma unroll
                for (int i = 0; i < 4; i++) accb[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(da[s][i], 1.f, accb[i], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                sum[i][r] += (double)acc[i][r];
                if (q == 0) sumb[i][r] += (double)accb[i][r];
            }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            hb[s] = hb_n[s];
#pragma unroll
            for (int i = 0; i < 4; i++) da[s][i] = da_n[s][i];
        }
    }
    float *out = partial + (size_t)slot * n_params;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (m0 + i >= L.nb) break;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int orow = 16 * (m0 + i) + 4 * k + r, ocol = 16 * q + j;
            if (orow < L.out_dim && ocol < L.in_dim) out[L.src_w + orow * L.in_dim + ocol] = (float)sum[i][r];
            if (q == 0 && j == 0 && orow < L.out_dim) out[L.src_b + orow] = (float)sumb[i][r];
        }
    }
}

__global__ void qg_policy_grad_reduce_kernel(KPolicy P, qg_ppo_params pp, int n, int n_slots, int n_params, const float *__restrict__ params,
                                             const float *__restrict__ partial, const double *__restrict__ slot_misc, float *__restrict__ grad,
                                             float *__restrict__ stats) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_params) {
        double s = 0.0;
        if (i >= P.src_log_std && i < P.src_log_std + P.act_dim) {
            for (int k = 0; k < n_slots; k++) s += slot_misc[(size_t)k * QGG_MISC + (i - P.src_log_std)];
            s -= (double)pp.ent_coef;
        } else {
            for (int k = 0; k < n_slots; k++) s += (double)partial[(size_t)k * n_params + i];
        }
        grad[i] = (float)s;
    } else if (stats && i < n_params + 8) {
        double sum[4] = {0.0, 0.0, 0.0, 0.0};          // QGG_MISC_POLICY .. QGG_MISC_VALUE: policy, kl, clip count, value
        for (int k = 0; k < n_slots; k++)
            for (int c = 0; c < 4; c++) sum[c] += slot_misc[(size_t)k * QGG_MISC + QGG_MISC_POLICY + c];
        double ent = 0.0;
        for (int a = 0; a < P.act_dim; a++) ent -= 0.5 + QGG_HALF_LOG_2PI + (double)params[P.src_log_std + a];
        const double b = (double)n;
        const double policy_loss = sum[0] / b, value_loss = sum[3] / b;
        const double v[8] = {policy_loss + (double)pp.ent_coef * ent + (double)pp.vf_coef * value_loss, policy_loss, value_loss, ent,
                             sum[1] / b, sum[2] / b, 0.0, 0.0};
        stats[i - n_params] = (float)v[i - n_params];
    }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
int qg_policy_pack_transposed(qg_policy *p, hipStream_t st) {
    if (!p->d_packed_t || p->g.packed_t_floats == 0) return QG_OK;
    const int threads = 256;
    qg_policy_pack_t_kernel<<<(p->g.packed_t_floats + threads - 1) / threads, threads, 0, st>>>(p->k, p->g, p->d_params, p->d_packed_t);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

// the row record, the transposed image and the work items of the weight-gradient launch: functions of the description alone
static void grad_layout(const KPolicy &k, KGrad *g) {
    memset(g, 0, sizeof *g);
    int rec = 0, wt = 0, item = 0;
    for (int t = 0; t < k.n_towers; t++)
        for (int l = 0; l < k.n_layers; l++) {
            const KPolLayer &L = k.layer[t][l];
            KGradLayer &GL = g->layer[t][l];
            GL.h_off = rec;
            GL.d_off = rec + 16 * L.nq;
            rec = GL.d_off + 16 * L.nb;
            GL.wt_off = wt;
            if (l > 0) wt += L.nb * L.nq * 256;
            GL.item0 = item;
            item += ((L.nb + 3) / 4) * L.nq;
        }
    g->rec = rec;
    g->packed_t_floats = wt;
    g->n_items = item + 1;
}

template <class T> static void grad_release(qg_policy *p, T *&ptr) {
    for (int i = 0; ptr && i < p->mem.count; i++)
        if (p->mem.ptr[i] == (void *)ptr) {
            (void)hipFree(ptr);
            p->mem.ptr[i] = p->mem.ptr[--p->mem.count];
            break;
        }
    ptr = nullptr;
}

extern "C" int qg_policy_reserve_grad(qg_policy *p, int32_t max_batch) {
    if (!p) return fail(QG_ERR_ARG, "qg_policy_reserve_grad: null policy");
    if (max_batch < 1) return fail(QG_ERR_ARG, "qg_policy_reserve_grad: max_batch must be >= 1");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);         // a pass on a caller's stream may be using what this replaces
    if (max_batch <= p->grad_max) return QG_OK;
    grad_layout(p->k, &p->g);
    const QgGradGeom geo = qg_policy_grad_geom(p, max_batch);
    const size_t tiles = geo.tiles, slots = geo.slots;
    p->grad_max = 0;
    grad_release(p, p->d_rec);
    grad_release(p, p->d_tile_misc);
    grad_release(p, p->d_slot_misc);
    grad_release(p, p->d_partial);
    if ((!p->d_packed_t && p->mem.alloc(p->d_packed_t, (size_t)p->g.packed_t_floats * sizeof(float))) ||
        p->mem.alloc(p->d_rec, tiles * QGP_TILE * (size_t)p->g.rec * sizeof(float)) ||
        p->mem.alloc(p->d_tile_misc, tiles * QGG_MISC * sizeof(double), true) ||
        p->mem.alloc(p->d_slot_misc, slots * QGG_MISC * sizeof(double), true) ||
        p->mem.alloc(p->d_partial, slots * (size_t)p->n_params * sizeof(float)))
        return QG_ERR_ALLOC;
    QG_TRY(qg_policy_pack_transposed(p, nullptr));
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    p->grad_max = max_batch;
    return QG_OK;
}

QgGradGeom qg_policy_grad_geom(const qg_policy *p, int32_t B) {
    const int tiles = (B - 1) / QGP_TILE + 1;          // B >= 1: ceil(B / QGP_TILE), whatever the size of B
    return {tiles, (tiles + QGG_SLOT_TILES - 1) / QGG_SLOT_TILES, (size_t)(p->k.lds0_floats + p->k.lds1_floats) * sizeof(float)};
}

int qg_policy_grad_check_rows(const qg_policy *p, const char *who, int32_t B, int32_t obs_stride, bool with_critic) {
    if (B < 1) return fail(QG_ERR_ARG, "%s: B must be >= 1", who);
    if (B > p->grad_max) return fail(QG_ERR_ARG, "%s: B = %d, but qg_policy_reserve_grad has reserved %d rows", who, B, p->grad_max);
    if (obs_stride < p->desc.obs_dim) return fail(QG_ERR_ARG, "%s: obs_stride %d < obs_dim %d", who, obs_stride, p->desc.obs_dim);
    if (obs_stride < qg_policy_row_width(p, with_critic))
        return fail(QG_ERR_ARG, "%s: obs_stride %d < %d, the end of the critic's window", who, obs_stride, qg_policy_row_width(p, with_critic));
    return QG_OK;
}

int qg_policy_grad_launch_weights(qg_policy *p, const KGrad &g, int tiles, int slots, hipStream_t st) {
    qg_policy_grad_weights_kernel<<<dim3((unsigned)g.n_items, (unsigned)slots), 64, 0, st>>>(p->k, g, tiles, p->n_params, p->d_rec, p->d_tile_misc,
                                                                                                p->d_partial, p->d_slot_misc);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_policy_ppo_grad_device(qg_policy *p, const qg_ppo_params *pp, int32_t B, const qg_ppo_batch *bt, float *grad, float *stats,
                                         void *stream) {
    if (!p || !pp || !bt || !grad) return fail(QG_ERR_ARG, "qg_policy_ppo_grad_device: null argument");
    QG_CHECK_STRUCT(pp, qg_ppo_params);
    QG_CHECK_STRUCT(bt, qg_ppo_batch);
    if (pp->reserved != 0) return fail(QG_ERR_ARG, "qg_ppo_params.reserved must be 0");
    if (!qg_finite32(pp->clip_range) || !(pp->clip_range > 0.f)) return fail(QG_ERR_ARG, "qg_ppo_params.clip_range must be finite and > 0");
    if (!qg_finite32(pp->clip_range_vf) || !qg_finite32(pp->ent_coef) || !qg_finite32(pp->vf_coef))
        return fail(QG_ERR_ARG, "qg_ppo_params: clip_range_vf, ent_coef and vf_coef must be finite");
    QG_TRY(qg_policy_grad_check_rows(p, "qg_policy_ppo_grad_device", B, bt->obs_stride, true));
    if (!bt->obs || !bt->actions || !bt->old_log_prob || !bt->advantages) return fail(QG_ERR_ARG, "qg_ppo_batch: null obs, actions, old_log_prob or advantages");
    if (p->desc.has_value && (!bt->returns || (pp->clip_range_vf > 0.f && !bt->old_values)))
        return fail(QG_ERR_ARG, "qg_ppo_batch: the policy has a critic: returns (and old_values when clip_range_vf > 0) are required");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    const hipStream_t st = (hipStream_t)stream;
    const QgGradGeom geo = qg_policy_grad_geom(p, B);
    qg_policy_grad_rows_kernel<<<dim3((unsigned)geo.tiles, (unsigned)p->k.n_towers), 64 * QGG_WAVES, geo.lds, st>>>(
        p->k, p->g, *pp, p->d_packed, p->d_packed_t, B, *bt, p->d_rec, p->d_tile_misc);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    QG_TRY(qg_policy_grad_launch_weights(p, p->g, geo.tiles, geo.slots, st));
    const int threads = 256;
    qg_policy_grad_reduce_kernel<<<(p->n_params + 8 + threads - 1) / threads, threads, 0, st>>>(p->k, *pp, B, geo.slots, p->n_params, p->d_params,
                                                                                                  p->d_partial, p->d_slot_misc, grad, stats);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}
