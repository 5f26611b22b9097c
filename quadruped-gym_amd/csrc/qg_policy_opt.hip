// qg_policy_opt.hip -- what stands between the PPO gradient and the next forward pass (include/quadgym.h: qg_policy_reserve_adam,
// qg_policy_adam_update_device, qg_policy_adam_get_state / _set_state, qg_policy_normalize_advantages_device).  DESIGN 4.13.
//
// An optimiser step is TWO launches, neither of which waits for another workgroup, and no atomics:
//   1. norm   -- a workgroup per slot of QGA_SLOT canonical elements: the f64 sum of squares of its part of the gradient (products of two
//                f32 are exact in f64; a thread adds its eight in ascending order, the wave a fixed butterfly, the four waves in
//                ascending order) into partial[slot].  Block 0 alone moves the step count t, which lives in device memory.
//   2. update -- the same partition.  One thread of every workgroup adds the partials in ascending order itself (norm, coef), one of
//                another wave forms the scalars that depend on t (lr / (1 - beta_one^t), sqrt(1 - beta_two^t): f64, rounded once), while
//                everybody's loads are in flight; then a thread updates its eight elements of p, m, v in f32 and scatters each new parameter straight to its place
//                in the forward image and, once qg_policy_reserve_grad has been called, in the transposed image: the inverse of the index
//                arithmetic of qg_policy_pack_kernel / qg_policy_pack_t_kernel.  A log_std element writes exp(log_std) (f64, rounded once)
//                and log_std.  Padding is never touched: it is zero from the pack launches of create / reserve_grad and stays zero.
// t is read by launch 2 only, after launch 1 has moved it: no workgroup sees a count another is about to change.
// Accesses on the canonical side are 16 bytes per lane where the caller's pointer is 16-byte aligned (the handle's own arrays are);
// which thread owns which element does not depend on that.
//
// The advantage normaliser is one launch of one workgroup: two passes in f64 (the mean, then the squares of the deviations), each a
// per-thread sum in ascending order, a fixed butterfly and the waves in ascending order, so the order depends on B alone.

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "qg_policy.h"

// four consecutive elements from index i (a multiple of 4); elements past n read as zero
__device__ __forceinline__ void qga_load4(const float *__restrict__ src, int i, int n, bool wide, float (&x)[4]) {
    if (wide && i + 3 < n) {
        const qgp_f32x4 q = *(const qgp_f32x4 *)(src + i);
        x[0] = q[0], x[1] = q[1], x[2] = q[2], x[3] = q[3];
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++) x[r] = i + r < n ? src[i + r] : 0.f;
    }
}

__device__ __forceinline__ void qga_store4(float *__restrict__ dst, int i, int n, bool wide, const float (&x)[4]) {
    if (wide && i + 3 < n) {
        *(qgp_f32x4 *)(dst + i) = qgp_f32x4{x[0], x[1], x[2], x[3]};
    } else {
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (i + r < n) dst[i + r] = x[r];
    }
}

// the sum over a workgroup: a fixed butterfly within the wave, then the waves in ascending order; the same value in every thread
template <int WAVES>
__device__ __forceinline__ double qga_block_sum(double s, double *ws) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
    __syncthreads();                                  // ws may still be read from the sum before
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    double total = 0.0;
    for (int w = 0; w < WAVES; w++) total += ws[w];
    return total;
}

constexpr int QGA_GROUPS = QGA_SLOT / (4 * QGA_THREADS);          // groups of four elements per thread

__global__ __launch_bounds__(QGA_THREADS) void qg_policy_adam_norm_kernel(int n, const float *__restrict__ grad, double *__restrict__ partial,
                                                                          long long *t) {
    __shared__ double ws[QGA_THREADS / 64];
    const bool wide = qg_aligned(grad, 16);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < QGA_GROUPS; k++) {
        float g[4];
        qga_load4(grad, blockIdx.x * QGA_SLOT + (k * QGA_THREADS + (int)threadIdx.x) * 4, n, wide, g);
#pragma unroll
        for (int r = 0; r < 4; r++) s += (double)g[r] * (double)g[r];
    }
    s = qga_block_sum<QGA_THREADS / 64>(s, ws);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = s;
        if (blockIdx.x == 0) *t += 1;
    }
}

// one element, in f32, in exactly this order (include/quadgym.h states it); nothing is contracted beyond the two fused multiply-adds
__device__ __forceinline__ void qga_element(float g, float coef, float b1, float omb1, float b2, float omb2, float step, float bc2s, float eps,
                                            float &p, float &m, float &v) {
#pragma clang fp contract(off)
    const float gc = coef * g;
    const float a = omb1 * gc;
    const float b = (omb2 * gc) * gc;
    m = fmaf(b1, m, a);
    v = fmaf(b2, v, b);
    const float denom = sqrtf(v) / bc2s + eps;
    const float q = m / denom;
    const float d = step * q;
    p = p - d;
}

// The canonical vector is a sequence of regions -- a layer's W, its b, .., log_std, the critic's layers --; a thread's four consecutive
// elements nearly always lie in one, so the region (and, in a W, the row and column) is looked up for the first and carried along.
// The layer table is read from LDS (QgaTable: filled once per workgroup; a scan of the kernel argument is a scalar load per layer).
#define QGA_REGION_W 0
#define QGA_REGION_B 1
#define QGA_REGION_LOG_STD 2
struct QgaTable {
    KPolLayer layer[2 * QGP_MAX_LAYERS];              // tower-major: the canonical order
    int32_t wt_off[2 * QGP_MAX_LAYERS];               // the layer's place in the transposed image; -1: it has none (layer 0, or no image)
};
struct QgaRegion {
    int kind, k, hi;                                  // which region, of which layer of the table; its end in the canonical vector
    int row, col;                                     // in a W: of the next element
};

__device__ __forceinline__ QgaRegion qga_find(const KPolicy &P, const QgaTable &T, int n_layers, int i) {
    QgaRegion r = {QGA_REGION_LOG_STD, 0, P.src_log_std + P.act_dim, 0, 0};
    if (i >= P.src_log_std && i < r.hi) return r;
    for (int k = 0; k < n_layers; k++) {
        const int sw = T.layer[k].src_w, sb = T.layer[k].src_b, in = T.layer[k].in_dim, out = T.layer[k].out_dim;
        if (i < sb) {                                  // (the regions ascend, and log_std has been dealt with: i >= sw)
            const int j = i - sw, row = j / in;
            return QgaRegion{QGA_REGION_W, k, sb, row, j - row * in};
        }
        if (i < sb + out) return QgaRegion{QGA_REGION_B, k, sb + out, 0, 0};
    }
    return r;                                          // not reached for i < n_params
}

// canonical element i has the new value x: its places in the two operand images
__device__ __forceinline__ void qga_scatter(const KPolicy &P, const QgaTable &T, int n_layers, QgaRegion &reg, int i, float x,
                                            float *__restrict__ packed, float *__restrict__ packed_t) {
    if (i >= reg.hi) reg = qga_find(P, T, n_layers, i);
    if (reg.kind == QGA_REGION_LOG_STD) {
        const int a = i - P.src_log_std;
        packed[P.std_off + a] = (float)exp((double)x);        // as qg_policy_pack_kernel: f64, rounded once
        packed[P.std_off + 16 + a] = x;
        return;
    }
    const KPolLayer &L = T.layer[reg.k];
    if (reg.kind == QGA_REGION_B) {
        packed[L.b_off + (i - L.src_b)] = x;
        return;
    }
    const int row = reg.row, col = reg.col, wt = T.wt_off[reg.k];
    // forward image W' [nb][nq][64][4]: row = 16 m + (lane & 15), col = 16 q + 4 (lane >> 4) + s
    packed[L.w_off + (((row >> 4) * L.nq + (col >> 4)) * 64 + ((col & 12) << 2) + (row & 15)) * 4 + (col & 3)] = x;
    // transposed image W^T' [nq][nb][64][4]: row = 16 mk + 4 (lane >> 4) + s, col = 16 qo + (lane & 15)
    if (wt >= 0) packed_t[wt + (((col >> 4) * L.nb + (row >> 4)) * 64 + ((row & 12) << 2) + (col & 15)) * 4 + (row & 3)] = x;
    if (++reg.col == L.in_dim) reg.col = 0, reg.row++;
}

__global__ __launch_bounds__(QGA_THREADS) void qg_policy_adam_update_kernel(KPolicy P, KGrad G, qg_adam_params ap, int n, int n_slots,
                                                                            const float *__restrict__ grad, const float *__restrict__ lr_device,
                                                                            const double *__restrict__ partial, const long long *__restrict__ t_dev,
                                                                            float *__restrict__ params, float *__restrict__ m_all,
                                                                            float *__restrict__ v_all, float *__restrict__ packed,
                                                                            float *__restrict__ packed_t, float *__restrict__ params_out,
                                                                            float *__restrict__ stats) {
    __shared__ float sc[3];
    __shared__ QgaTable table;
    const int n_layers = P.n_towers * P.n_layers;
    if ((int)threadIdx.x < n_layers) {
        const int t = threadIdx.x / P.n_layers, l = threadIdx.x - t * P.n_layers;
        table.layer[threadIdx.x] = P.layer[t][l];
        table.wt_off[threadIdx.x] = (packed_t && l > 0) ? G.layer[t][l].wt_off : -1;
    }
    const bool wide_g = qg_aligned(grad, 16), wide_o = qg_aligned(params_out, 16);
    float g[QGA_GROUPS][4], p[QGA_GROUPS][4], m[QGA_GROUPS][4], v[QGA_GROUPS][4];
#pragma unroll
    for (int k = 0; k < QGA_GROUPS; k++) {
        const int i = blockIdx.x * QGA_SLOT + (k * QGA_THREADS + (int)threadIdx.x) * 4;
        qga_load4(grad, i, n, wide_g, g[k]);
        qga_load4(params, i, n, true, p[k]);
        qga_load4(m_all, i, n, true, m[k]);
        qga_load4(v_all, i, n, true, v[k]);
    }
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int k = 0; k < n_slots; k++) sum += partial[k];
        const float norm = (float)sqrt(sum);
        float coef = 1.f;
        if (ap.max_grad_norm > 0.f) coef = fminf(1.f, ap.max_grad_norm / (norm + 1e-6f));
        sc[0] = coef;
        if (blockIdx.x == 0 && stats) stats[0] = norm, stats[1] = coef;
    } else if (threadIdx.x == 64) {                   // another wave: the scalars that depend on t, beside the sum of the partials
        const long long t = *t_dev;
        const float lr = lr_device ? *lr_device : ap.lr;
        const double bc1 = 1.0 - pow((double)ap.beta_one, (double)t), bc2 = 1.0 - pow((double)ap.beta_two, (double)t);
        sc[1] = (float)((double)lr / bc1);
        sc[2] = (float)sqrt(bc2);
        if (blockIdx.x == 0 && stats) stats[2] = (float)t, stats[3] = lr;
    }
    __syncthreads();
    const float coef = sc[0], step = sc[1], bc2s = sc[2];
    const float omb1 = (float)(1.0 - (double)ap.beta_one), omb2 = (float)(1.0 - (double)ap.beta_two);
#pragma unroll
    for (int k = 0; k < QGA_GROUPS; k++) {
        const int i = blockIdx.x * QGA_SLOT + (k * QGA_THREADS + (int)threadIdx.x) * 4;
        if (i >= n) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) qga_element(g[k][r], coef, ap.beta_one, omb1, ap.beta_two, omb2, step, bc2s, ap.eps, p[k][r], m[k][r], v[k][r]);
        qga_store4(params, i, n, true, p[k]);
        qga_store4(m_all, i, n, true, m[k]);
        qga_store4(v_all, i, n, true, v[k]);
        if (params_out) qga_store4(params_out, i, n, wide_o, p[k]);
        QgaRegion reg = {0, 0, 0, 0, 0};                  // hi = 0: the group's first element looks its region up
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (i + r < n) qga_scatter(P, table, n_layers, reg, i + r, p[k][r], packed, packed_t);
    }
}

// SB3's normalize_advantage.  Thread t owns the groups of four elements t, t + QGN_THREADS, .. whatever the width of its loads.
__global__ __launch_bounds__(QGN_THREADS) void qg_policy_normalize_advantages_kernel(int n, const float *adv, float *out) {
    __shared__ double ws[QGN_THREADS / 64];
    const bool wide_in = qg_aligned(adv, 16), wide_out = qg_aligned(out, 16);
    double s = 0.0;
    for (int i = 4 * (int)threadIdx.x; i < n; i += 4 * QGN_THREADS) {
        float x[4];
        qga_load4(adv, i, n, wide_in, x);
#pragma unroll
        for (int r = 0; r < 4; r++) s += (double)x[r];
    }
    const double mean = qga_block_sum<QGN_THREADS / 64>(s, ws) / (double)n;
    s = 0.0;
    for (int i = 4 * (int)threadIdx.x; i < n; i += 4 * QGN_THREADS) {
        float x[4];
        qga_load4(adv, i, n, wide_in, x);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double d = i + r < n ? (double)x[r] - mean : 0.0;
            s += d * d;
        }
    }
    // (every thread has read what it needs of adv for the sums before any thread writes: the barriers of the block sum)
    const double scale = sqrt(qga_block_sum<QGN_THREADS / 64>(s, ws) / (double)(n - 1)) + 1e-8;
    for (int i = 4 * (int)threadIdx.x; i < n; i += 4 * QGN_THREADS) {
        float x[4], y[4];
        qga_load4(adv, i, n, wide_in, x);
#pragma unroll
        for (int r = 0; r < 4; r++) y[r] = (float)(((double)x[r] - mean) / scale);
        qga_store4(out, i, n, wide_out, y);
    }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
extern "C" int qg_policy_reserve_adam(qg_policy *p) {
    if (!p) return fail(QG_ERR_ARG, "qg_policy_reserve_adam: null policy");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    if (p->adam_slots) return QG_OK;
    const int slots = (p->n_params + QGA_SLOT - 1) / QGA_SLOT;
    if (p->mem.alloc(p->d_adam_m, (size_t)p->n_params * sizeof(float), true) || p->mem.alloc(p->d_adam_v, (size_t)p->n_params * sizeof(float), true) ||
        p->mem.alloc(p->d_adam_t, sizeof(long long), true) || p->mem.alloc(p->d_adam_partial, (size_t)slots * sizeof(double), true))
        return QG_ERR_ALLOC;
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    p->adam_slots = slots;
    return QG_OK;
}

static bool unit_interval(float x) { return qg_finite32(x) && x >= 0.f && x < 1.f; }

extern "C" int qg_policy_adam_update_device(qg_policy *p, const qg_adam_params *ap, const float *grad, const float *lr_device, float *params_out,
                                          float *stats, void *stream) {
    if (!p || !ap || !grad) return fail(QG_ERR_ARG, "qg_policy_adam_update_device: null argument");
    QG_CHECK_STRUCT(ap, qg_adam_params);
    if (ap->reserved != 0) return fail(QG_ERR_ARG, "qg_adam_params.reserved must be 0");
    if (!qg_finite32(ap->lr) || !(ap->lr >= 0.f)) return fail(QG_ERR_ARG, "qg_adam_params.lr must be finite and >= 0");
    if (!unit_interval(ap->beta_one) || !unit_interval(ap->beta_two)) return fail(QG_ERR_ARG, "qg_adam_params: beta_one and beta_two must lie in [0, 1)");
    if (!qg_finite32(ap->eps) || !(ap->eps > 0.f)) return fail(QG_ERR_ARG, "qg_adam_params.eps must be finite and > 0");
    if (!qg_finite32(ap->max_grad_norm)) return fail(QG_ERR_ARG, "qg_adam_params.max_grad_norm must be finite (<= 0: clipping off)");
    if (params_out == grad) return fail(QG_ERR_ARG, "qg_policy_adam_update_device: params_out must not be grad");
    if (!p->adam_slots) return fail(QG_ERR_ARG, "qg_policy_adam_update_device: qg_policy_reserve_adam has not been called");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    const hipStream_t st = (hipStream_t)stream;
    qg_policy_adam_norm_kernel<<<p->adam_slots, QGA_THREADS, 0, st>>>(p->n_params, grad, p->d_adam_partial, p->d_adam_t);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    qg_policy_adam_update_kernel<<<p->adam_slots, QGA_THREADS, 0, st>>>(p->k, p->g, *ap, p->n_params, p->adam_slots, grad, lr_device, p->d_adam_partial,
                                                                        p->d_adam_t, p->d_params, p->d_adam_m, p->d_adam_v, p->d_packed, p->d_packed_t,
                                                                        params_out, stats);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_policy_adam_get_state(qg_policy *p, float *exp_avg, float *exp_avg_sq, int64_t *step) {
    if (!p || !exp_avg || !exp_avg_sq || !step) return fail(QG_ERR_ARG, "qg_policy_adam_get_state: null argument");
    if (!p->adam_slots) return fail(QG_ERR_ARG, "qg_policy_adam_get_state: qg_policy_reserve_adam has not been called");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);         // a step may be in flight on a caller's stream
    const size_t bytes = (size_t)p->n_params * sizeof(float);
    long long t = 0;
    HIP_TRY(hipMemcpy(exp_avg, p->d_adam_m, bytes, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(exp_avg_sq, p->d_adam_v, bytes, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(&t, p->d_adam_t, sizeof t, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    *step = (int64_t)t;
    return QG_OK;
}

extern "C" int qg_policy_adam_set_state(qg_policy *p, const float *exp_avg, const float *exp_avg_sq, int64_t step) {
    if (!p || !exp_avg || !exp_avg_sq) return fail(QG_ERR_ARG, "qg_policy_adam_set_state: null argument");
    if (step < 0) return fail(QG_ERR_ARG, "qg_policy_adam_set_state: step must be >= 0");
    if (!p->adam_slots) return fail(QG_ERR_ARG, "qg_policy_adam_set_state: qg_policy_reserve_adam has not been called");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    const size_t bytes = (size_t)p->n_params * sizeof(float);
    const long long t = (long long)step;
    HIP_TRY(hipMemcpy(p->d_adam_m, exp_avg, bytes, hipMemcpyHostToDevice), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(p->d_adam_v, exp_avg_sq, bytes, hipMemcpyHostToDevice), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(p->d_adam_t, &t, sizeof t, hipMemcpyHostToDevice), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_policy_normalize_advantages_device(qg_policy *p, int32_t B, const float *adv, float *out, void *stream) {
    if (!p || !adv || !out) return fail(QG_ERR_ARG, "qg_policy_normalize_advantages_device: null argument");
    if (B < 2) return fail(QG_ERR_ARG, "qg_policy_normalize_advantages_device: B must be >= 2 (the standard deviation of one row is undefined)");
    if (B > INT32_MAX - 4 * QGN_THREADS) return fail(QG_ERR_ARG, "qg_policy_normalize_advantages_device: B must be <= %d", INT32_MAX - 4 * QGN_THREADS);
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    qg_policy_normalize_advantages_kernel<<<1, QGN_THREADS, 0, (hipStream_t)stream>>>(B, adv, out);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}
