// qg_norm.hip -- running observation and reward normalisation (include/quadgym.h: qg_norm_*): SB3's VecNormalize on rows that are
// already on the device.  A training step is THREE launches:
//
//   qg_norm_moments_kernel   per tile of R rows and 64 columns: (mean, M2) of the tile in f64 -> one slab entry per (tile, column).
//                            One more row of blocks advances the return accumulator (returns = returns * gamma + reward) and
//                            produces the same pair for it: the returns are column obs_dim of every table here.
//   qg_norm_combine_kernel   per column: the tiles' pairs merged in a fixed order that depends on (n, D) alone, then the running
//                            merge; writes mean, var, count and 1 / sqrt(var + epsilon).
//   qg_norm_apply_kernel     out = clip(f32((f64(x) - mean) * inv_std)); the reward likewise; returns[done] = 0.
//
// No floating-point atomics and no workgroup ever waits for, or reads what was written by, another workgroup of its own launch: what
// passes from one stage to the next passes through a kernel boundary.  Within a launch the read set and the written set are
// disjoint but for words one thread both reads and writes (its column's statistics, its env's return, its element in place).
//
// Layout.  Lanes run along the columns (a wave's load of a row segment is 256 contiguous bytes), the four waves of a workgroup take
// the rows of a tile in turn.  Statistics: f64 [4][obs_dim + 1] = mean | var | count | inv_std, the count kept per column so that a
// column's thread owns every word it updates.
//
// Numerics.  f64 moments, K a thread's first element of its tile; everything above a thread is Chan's merge (qg_moments_dev.h).

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>
#include <cstring>

#include "qg_host.h"
#include "qg_moments_dev.h"

#define QGN_COLS 64               // columns per workgroup of the moments pass (one per lane)
#define QGN_WAVES 4
#define QGN_MAX_TILES 512         // slab entries per column; the rows per tile grow with n so that this holds
#define QGN_SLICES 16             // the combine pass merges the tiles in 16 runs per column, then a tree over the runs

typedef float qgn_f32x4 __attribute__((ext_vector_type(4)));

// the one expression of the reciprocal standard deviation (the combine pass and qg_norm_set_state both go through it, so a
// restored state normalises with the bits the original did)
__device__ __forceinline__ double qgn_inv_std(double var, double eps) {
#pragma clang fp contract(off)
    const double v = var + eps;
    return 1.0 / sqrt(v);
}

__global__ __launch_bounds__(64) void qg_norm_inv_kernel(int Dp, double *__restrict__ stats, double eps) {
    for (int c = threadIdx.x; c < Dp; c += 64) stats[3 * Dp + c] = qgn_inv_std(stats[Dp + c], eps);
}

// grid (tiles, column chunks [+ 1]); blockIdx.y + y0 == nchunk is the return accumulator's row of blocks
__global__ __launch_bounds__(64 * QGN_WAVES) void qg_norm_moments_kernel(int n, int D, int R, int nchunk, int y0,
                                                                         const float *__restrict__ obs, int stride,
                                                                         const float *__restrict__ reward, int rstride,
                                                                         double *__restrict__ returns, double gamma,
                                                                         double2 *__restrict__ part) {
    __shared__ double sh[3][64 * QGN_WAVES];
    const int Dp = D + 1;
    const int g = blockIdx.x, chunk = blockIdx.y + y0;
    const int row0 = g * R, rows = min(R, n - row0);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double cnt = 0.0, K = 0.0, s1 = 0.0, s2 = 0.0;

    if (chunk < nchunk) {
        const int c = QGN_COLS * chunk + lane;
        const float *col = obs + min(c, D - 1);
        constexpr int U = 4;
        for (int r = wave; r < rows; r += QGN_WAVES * U) {
            float x[U];
#pragma unroll
            for (int u = 0; u < U; u++) x[u] = col[(size_t)(row0 + min(r + QGN_WAVES * u, rows - 1)) * stride];
#pragma unroll
            for (int u = 0; u < U; u++)
                if (r + QGN_WAVES * u < rows) {
                    if (cnt == 0.0) K = (double)x[u];
                    const double d = (double)x[u] - K;
                    s1 += d;
                    s2 += d * d;
                    cnt += 1.0;
                }
        }
        double mean, M2;
        qg_moments_finish(cnt, K, s1, s2, mean, M2);
        sh[0][t] = cnt, sh[1][t] = mean, sh[2][t] = M2;
        __syncthreads();
        if (wave == 0) {
            for (int w = 1; w < QGN_WAVES; w++) qg_moments_merge(cnt, mean, M2, sh[0][64 * w + lane], sh[1][64 * w + lane], sh[2][64 * w + lane]);
            if (c < D) part[(size_t)g * Dp + c] = make_double2(mean, M2);
        }
    } else {
        // the returns: a thread takes the envs t, t + 256, .. of the tile
        for (int r = t; r < rows; r += 64 * QGN_WAVES) {
            const size_t i = (size_t)(row0 + r);
            const double ret = returns[i] * gamma + (double)reward[i * rstride];
            returns[i] = ret;
            if (cnt == 0.0) K = ret;
            const double d = ret - K;
            s1 += d;
            s2 += d * d;
            cnt += 1.0;
        }
        double mean, M2;
        qg_moments_finish(cnt, K, s1, s2, mean, M2);
        sh[0][t] = cnt, sh[1][t] = mean, sh[2][t] = M2;
        __syncthreads();
        for (int off = 32 * QGN_WAVES; off >= 1; off >>= 1) {
            if (t < off) {
                qg_moments_merge(cnt, mean, M2, sh[0][t + off], sh[1][t + off], sh[2][t + off]);
                sh[0][t] = cnt, sh[1][t] = mean, sh[2][t] = M2;
            }
            __syncthreads();
        }
        if (t == 0) part[(size_t)g * Dp + D] = make_double2(mean, M2);
    }
}

// columns c_lo .. c_hi - 1 (the returns are column D), 16 per workgroup; thread (s, cc) merges run s of column cc's tiles
__global__ __launch_bounds__(16 * QGN_SLICES) void qg_norm_combine_kernel(int n, int R, int G, int Dp, int c_lo, int c_hi,
                                                                         const double2 *__restrict__ part, double *__restrict__ stats,
                                                                         double eps) {
    __shared__ double sh[3][16 * QGN_SLICES];
    const int t = threadIdx.x, cc = t & 15, s = t >> 4;
    const int c = c_lo + 16 * blockIdx.x + cc;
    const bool active = c < c_hi;
    const int cr = min(c, c_hi - 1);
    const int GS = (G + QGN_SLICES - 1) / QGN_SLICES;
    const int g1 = min(G, (s + 1) * GS);
    double na = 0.0, ma = 0.0, Ma = 0.0;
    for (int g = s * GS; g < g1; g++) {
        const double2 p = part[(size_t)g * Dp + cr];
        qg_moments_merge(na, ma, Ma, (double)min(R, n - g * R), p.x, p.y);
    }
    sh[0][t] = na, sh[1][t] = ma, sh[2][t] = Ma;
    __syncthreads();
    for (int off = QGN_SLICES / 2; off >= 1; off >>= 1) {
        if (s < off) {
            qg_moments_merge(na, ma, Ma, sh[0][t + 16 * off], sh[1][t + 16 * off], sh[2][t + 16 * off]);
            sh[0][t] = na, sh[1][t] = ma, sh[2][t] = Ma;
        }
        __syncthreads();
    }
    if (s == 0 && active) {
        // RunningMeanStd.update_from_moments: bm = ma, bv * n = Ma
        const double mean = stats[c], var = stats[Dp + c], count = stats[2 * Dp + c];
        const double delta = ma - mean, tot = count + na;
        const double mean1 = mean + delta * na / tot;
        const double M2 = var * count + Ma + delta * delta * count * na / tot;
        const double var1 = M2 / tot;
        stats[c] = mean1;
        stats[Dp + c] = var1;
        stats[2 * Dp + c] = tot;
        stats[3 * Dp + c] = qgn_inv_std(var1, eps);
    }
}

struct KNormApply {
    int32_t n, D, Dp;
    int32_t in_stride, out_stride;
    int32_t obs_blocks;            // blocks [0, obs_blocks) take the observations, the rest the rewards
    int32_t norm_obs, norm_reward;
    int32_t rin_stride, rout_stride;
    int32_t done_kind, done_stride;
    int32_t zero_returns;
    float clip_obs, clip_reward;
};

__device__ __forceinline__ float qgn_norm1(float x, double mean, double inv, float clip) {
    const float y = (float)(((double)x - mean) * inv);          // rounded to f32 once, then clipped
    return fminf(fmaxf(y, -clip), clip);
}

// VEC: 16 bytes per lane (obs_dim, both strides and both bases are multiples of four floats)
template <bool VEC>
__global__ __launch_bounds__(256) void qg_norm_apply_kernel(KNormApply A, const float *obs_in, float *obs_out, const double *__restrict__ stats,
                                                            const float *reward_in, float *reward_out, const void *done,
                                                            double *__restrict__ returns) {
    if ((int)blockIdx.x < A.obs_blocks) {
        constexpr int W = VEC ? 4 : 1;
        const uint32_t per_row = (uint32_t)(A.D / W);
        const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x, total = (uint64_t)A.n * per_row;
        if (idx >= total) return;
        uint32_t row, cv;
        if (total <= 0xffffffffull) {
            row = (uint32_t)idx / per_row;
            cv = (uint32_t)idx - row * per_row;
        } else {
            row = (uint32_t)(idx / per_row);
            cv = (uint32_t)(idx - (uint64_t)row * per_row);
        }
        const int c = (int)cv * W;
        const float *src = obs_in + (size_t)row * A.in_stride + c;
        float *dst = obs_out + (size_t)row * A.out_stride + c;
        if constexpr (VEC) {
            qgn_f32x4 v = *(const qgn_f32x4 *)src;
            if (A.norm_obs) {
#pragma unroll
                for (int k = 0; k < 4; k++) v[k] = qgn_norm1(v[k], stats[c + k], stats[3 * A.Dp + c + k], A.clip_obs);
            }
            *(qgn_f32x4 *)dst = v;
        } else {
            float v = *src;
            if (A.norm_obs) v = qgn_norm1(v, stats[c], stats[3 * A.Dp + c], A.clip_obs);
            *dst = v;
        }
    } else {
        const uint64_t i = (uint64_t)(blockIdx.x - A.obs_blocks) * 256 + threadIdx.x;
        if (i >= (uint64_t)A.n) return;
        float r = reward_in[i * A.rin_stride];
        if (A.norm_reward) r = qgn_norm1(r, 0.0, stats[3 * A.Dp + A.D], A.clip_reward);
        reward_out[i * A.rout_stride] = r;
        if (A.zero_returns) {
            if (qg_done_at(done, A.done_kind, A.done_stride, i)) returns[i] = 0.0;
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
struct qg_norm {
    int32_t device;
    qg_norm_desc desc;
    int32_t Dp;               // obs_dim + 1: the returns are the last column of every table
    QgDevMem mem;
    double *d_stats;          // [4][Dp]: mean | var | count | 1 / sqrt(var + epsilon)
    double *d_returns;        // [n_envs]
    double2 *d_part;          // [QGN_MAX_TILES][Dp]: the moments pass's (mean, M2) per tile and column
};

static int norm_validate(const qg_norm_desc *d) {
    if (!d) return fail(QG_ERR_ARG, "qg_norm: null description");
    QG_CHECK_STRUCT(d, qg_norm_desc);
    if (d->obs_dim < 1 || d->obs_dim > 512) return fail(QG_ERR_ARG, "qg_norm: obs_dim %d outside 1 .. 512", d->obs_dim);
    if (d->n_envs < 1) return fail(QG_ERR_ARG, "qg_norm: n_envs %d must be >= 1", d->n_envs);
    if (!qg_finite64(d->gamma) || d->gamma < 0.0) return fail(QG_ERR_ARG, "qg_norm: gamma %g must be finite and >= 0", d->gamma);
    if (!qg_finite64(d->epsilon) || d->epsilon < 0.0) return fail(QG_ERR_ARG, "qg_norm: epsilon %g must be finite and >= 0", d->epsilon);
    if (!qg_finite64(d->clip_obs) || d->clip_obs <= 0.0) return fail(QG_ERR_ARG, "qg_norm: clip_obs %g must be finite and > 0", d->clip_obs);
    if (!qg_finite64(d->clip_reward) || d->clip_reward <= 0.0)
        return fail(QG_ERR_ARG, "qg_norm: clip_reward %g must be finite and > 0", d->clip_reward);
    if ((d->norm_obs != 0 && d->norm_obs != 1) || (d->norm_reward != 0 && d->norm_reward != 1))
        return fail(QG_ERR_ARG, "qg_norm: norm_obs and norm_reward are 0 or 1");
    return QG_OK;
}

extern "C" int qg_norm_destroy(qg_norm *p) {
    if (p) qg_free_handle(p, p->device);           // steps may still be in flight on a caller's stream
    return QG_OK;
}

// mean 0, var 1, count 1e-4 for the observations and the returns; returns 0
static int norm_upload(qg_norm *p, const double *mean, const double *var, const double *count, double ret_mean, double ret_var,
                       double ret_count, const double *returns) {
    const int D = p->desc.obs_dim, Dp = p->Dp;
    QgHostBuf<double> h((size_t)4 * Dp);
    QG_TRY(h.oom());
    for (int c = 0; c < D; c++) h[c] = mean ? mean[c] : 0.0, h[Dp + c] = var ? var[c] : 1.0, h[2 * Dp + c] = count ? *count : 1e-4;
    h[D] = ret_mean, h[Dp + D] = ret_var, h[2 * Dp + D] = ret_count;
    for (int c = 0; c < Dp; c++) h[3 * Dp + c] = 0.0;
    HIP_TRY(hipMemcpy(p->d_stats, h, (size_t)4 * Dp * sizeof(double), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    if (returns) HIP_TRY(hipMemcpy(p->d_returns, returns, (size_t)p->desc.n_envs * sizeof(double), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    else HIP_TRY(hipMemset(p->d_returns, 0, (size_t)p->desc.n_envs * sizeof(double)), QG_ERR_DEVICE);
    qg_norm_inv_kernel<<<1, 64, 0, nullptr>>>(Dp, p->d_stats, p->desc.epsilon);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_norm_create(int32_t device_id, const qg_norm_desc *desc, qg_norm **out) {
    if (!out) return fail(QG_ERR_ARG, "qg_norm_create: null output");
    *out = nullptr;
    QG_TRY(norm_validate(desc));
    QG_TRY(qg_open_device(device_id, nullptr));
    qg_norm *p = qg_new_handle<qg_norm>();
    if (!p) return QG_ERR_ALLOC;
    p->device = device_id;
    p->desc = *desc;
    p->Dp = desc->obs_dim + 1;
    if (p->mem.alloc(p->d_stats, (size_t)4 * p->Dp * sizeof(double)) || p->mem.alloc(p->d_returns, (size_t)desc->n_envs * sizeof(double)) ||
        p->mem.alloc(p->d_part, (size_t)QGN_MAX_TILES * p->Dp * sizeof(double2))) {
        qg_norm_destroy(p);
        return QG_ERR_ALLOC;
    }
    const int rc = norm_upload(p, nullptr, nullptr, nullptr, 0.0, 1.0, 1e-4, nullptr);
    if (rc != QG_OK) {
        qg_norm_destroy(p);
        return rc;
    }
    *out = p;
    return QG_OK;
}

// rows per tile of the moments pass: 16, or what keeps n rows within QGN_MAX_TILES tiles (a multiple of the four waves)
static int norm_tile_rows(int32_t n) {
    const int r = (int)(((int64_t)n + QGN_MAX_TILES - 1) / QGN_MAX_TILES);
    return r <= 16 ? 16 : (r + QGN_WAVES - 1) / QGN_WAVES * QGN_WAVES;
}

// steps 1 and 3: the moments of obs (when given) and of the advanced returns (when reward is given), merged into the statistics
static int norm_update(qg_norm *p, int32_t n, const float *obs, int32_t stride, const float *reward, int32_t rstride, hipStream_t st) {
    if (!obs && !reward) return QG_OK;
    const int D = p->desc.obs_dim, R = norm_tile_rows(n), G = (n + R - 1) / R;
    const int nchunk = (D + QGN_COLS - 1) / QGN_COLS;
    const dim3 grid((unsigned)G, (unsigned)((obs ? nchunk : 0) + (reward ? 1 : 0)));
    qg_norm_moments_kernel<<<grid, 64 * QGN_WAVES, 0, st>>>(n, D, R, nchunk, obs ? 0 : nchunk, obs, stride, reward, rstride, p->d_returns,
                                                           p->desc.gamma, p->d_part);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    const int c_lo = obs ? 0 : D, c_hi = reward ? D + 1 : D;
    qg_norm_combine_kernel<<<(c_hi - c_lo + 15) / 16, 16 * QGN_SLICES, 0, st>>>(n, R, G, p->Dp, c_lo, c_hi, p->d_part, p->d_stats, p->desc.epsilon);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

// steps 2, 4 and 5
static int norm_apply(qg_norm *p, int32_t n, const float *obs_in, int32_t in_stride, float *obs_out, int32_t out_stride, const float *reward_in,
                      int32_t rin_stride, float *reward_out, int32_t rout_stride, const void *done, int32_t done_kind, int32_t done_stride,
                      bool zero_returns, hipStream_t st) {
    const int D = p->desc.obs_dim;
    KNormApply A;
    memset(&A, 0, sizeof A);
    A.n = n, A.D = D, A.Dp = p->Dp;
    A.in_stride = in_stride, A.out_stride = out_stride;
    A.norm_obs = p->desc.norm_obs, A.norm_reward = p->desc.norm_reward;
    A.rin_stride = rin_stride, A.rout_stride = rout_stride;
    A.done_kind = done_kind, A.done_stride = done_stride;
    A.zero_returns = zero_returns && done;
    A.clip_obs = (float)p->desc.clip_obs, A.clip_reward = (float)p->desc.clip_reward;
    const bool vec = D % 4 == 0 && in_stride % 4 == 0 && out_stride % 4 == 0 && qg_aligned(obs_in, 16) && qg_aligned(obs_out, 16);
    const bool obs_work = obs_in && (A.norm_obs || obs_in != obs_out);          // switched off and in place: nothing to copy
    const bool rew_work = reward_in && (A.norm_reward || reward_in != reward_out || A.zero_returns);
    const int64_t obs_items = obs_work ? (int64_t)n * (D / (vec ? 4 : 1)) : 0;
    const int64_t blocks = (obs_items + 255) / 256 + (rew_work ? ((int64_t)n + 255) / 256 : 0);
    if (blocks == 0) return QG_OK;
    if (blocks > INT32_MAX) return fail(QG_ERR_ARG, "qg_norm: %d rows of %d columns are more than one launch takes", n, D);
    A.obs_blocks = (int32_t)((obs_items + 255) / 256);
    if (vec) qg_norm_apply_kernel<true><<<(unsigned)blocks, 256, 0, st>>>(A, obs_in, obs_out, p->d_stats, reward_in, reward_out, done, p->d_returns);
    else qg_norm_apply_kernel<false><<<(unsigned)blocks, 256, 0, st>>>(A, obs_in, obs_out, p->d_stats, reward_in, reward_out, done, p->d_returns);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_norm_step_device(qg_norm *p, int32_t n, const float *obs_in, int32_t in_stride, float *obs_out, int32_t out_stride,
                                   const float *reward_in, int32_t reward_in_stride, float *reward_out, int32_t reward_out_stride,
                                   const void *done, int32_t done_kind, int32_t done_stride, int32_t training, void *stream) {
    if (!p || !obs_in || !obs_out) return fail(QG_ERR_ARG, "qg_norm_step_device: null argument");
    if (n != p->desc.n_envs) return fail(QG_ERR_ARG, "qg_norm_step_device: n is %d, the handle was built for %d envs", n, p->desc.n_envs);
    if (in_stride < p->desc.obs_dim || out_stride < p->desc.obs_dim)
        return fail(QG_ERR_ARG, "qg_norm_step_device: strides %d, %d < obs_dim %d", in_stride, out_stride, p->desc.obs_dim);
    if (reward_in) {
        if (!reward_out) return fail(QG_ERR_ARG, "qg_norm_step_device: reward_in without reward_out");
        if (reward_in_stride < 1 || reward_out_stride < 1) return fail(QG_ERR_ARG, "qg_norm_step_device: reward strides must be >= 1");
        QG_TRY(qg_check_done("qg_norm_step_device", done, done_kind, done_stride));
    }
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    const hipStream_t st = (hipStream_t)stream;
    if (training) QG_TRY(norm_update(p, n, p->desc.norm_obs ? obs_in : nullptr, in_stride, reward_in, reward_in_stride, st));
    return norm_apply(p, n, obs_in, in_stride, obs_out, out_stride, reward_in, reward_in_stride, reward_out, reward_out_stride,
                      reward_in ? done : nullptr, done_kind, done_stride, training != 0, st);
}

extern "C" int qg_norm_update_obs_device(qg_norm *p, int32_t n, const float *obs, int32_t stride, void *stream) {
    if (!p || !obs) return fail(QG_ERR_ARG, "qg_norm_update_obs_device: null argument");
    if (n < 1) return fail(QG_ERR_ARG, "qg_norm_update_obs_device: n must be >= 1");
    if (stride < p->desc.obs_dim) return fail(QG_ERR_ARG, "qg_norm_update_obs_device: stride %d < obs_dim %d", stride, p->desc.obs_dim);
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    return norm_update(p, n, obs, stride, nullptr, 0, (hipStream_t)stream);
}

extern "C" int qg_norm_apply_obs_device(qg_norm *p, int32_t n, const float *obs_in, int32_t in_stride, float *obs_out, int32_t out_stride,
                                        void *stream) {
    if (!p || !obs_in || !obs_out) return fail(QG_ERR_ARG, "qg_norm_apply_obs_device: null argument");
    if (n < 1) return fail(QG_ERR_ARG, "qg_norm_apply_obs_device: n must be >= 1");
    if (in_stride < p->desc.obs_dim || out_stride < p->desc.obs_dim)
        return fail(QG_ERR_ARG, "qg_norm_apply_obs_device: strides %d, %d < obs_dim %d", in_stride, out_stride, p->desc.obs_dim);
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    return norm_apply(p, n, obs_in, in_stride, obs_out, out_stride, nullptr, 0, nullptr, 0, nullptr, 0, 0, false, (hipStream_t)stream);
}

extern "C" int qg_norm_reset_returns_device(qg_norm *p, void *stream) {
    if (!p) return fail(QG_ERR_ARG, "qg_norm_reset_returns_device: null argument");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipMemsetAsync(p->d_returns, 0, (size_t)p->desc.n_envs * sizeof(double), (hipStream_t)stream), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_norm_get_state(qg_norm *p, double *mean, double *var, double *count, double *ret_mean, double *ret_var, double *ret_count,
                                 double *returns) {
    if (!p || !mean || !var || !count || !ret_mean || !ret_var || !ret_count || !returns)
        return fail(QG_ERR_ARG, "qg_norm_get_state: null argument");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);         // a step may be in flight on a caller's stream
    const int D = p->desc.obs_dim, Dp = p->Dp;
    QgHostBuf<double> h((size_t)3 * Dp);
    QG_TRY(h.oom());
    HIP_TRY(hipMemcpy(h, p->d_stats, (size_t)3 * Dp * sizeof(double), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(returns, p->d_returns, (size_t)p->desc.n_envs * sizeof(double), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    memcpy(mean, h, (size_t)D * sizeof(double));
    memcpy(var, h + Dp, (size_t)D * sizeof(double));
    *count = h[2 * Dp];
    *ret_mean = h[D], *ret_var = h[Dp + D], *ret_count = h[2 * Dp + D];
    return QG_OK;
}

extern "C" int qg_norm_set_state(qg_norm *p, const double *mean, const double *var, double count, double ret_mean, double ret_var,
                                 double ret_count, const double *returns) {
    if (!p || !mean || !var || !returns) return fail(QG_ERR_ARG, "qg_norm_set_state: null argument");
    for (int c = 0; c < p->desc.obs_dim; c++)
        if (!qg_finite64(mean[c]) || !qg_finite64(var[c]) || var[c] < 0.0)
            return fail(QG_ERR_ARG, "qg_norm_set_state: column %d: mean %g, var %g (finite, var >= 0)", c, mean[c], var[c]);
    if (!qg_finite64(count) || count <= 0.0 || !qg_finite64(ret_count) || ret_count <= 0.0 || !qg_finite64(ret_mean) ||
        !qg_finite64(ret_var) || ret_var < 0.0)
        return fail(QG_ERR_ARG, "qg_norm_set_state: counts must be > 0, the return statistic finite with var >= 0");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    return norm_upload(p, mean, var, &count, ret_mean, ret_var, ret_count, returns);
}
