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
// Numerics.  Within a tile a thread accumulates sum(x - K) and sum((x - K)^2) in f64 with K its first element (x - K is exact in
// f64 for f32 inputs; a constant column gives M2 = 0 exactly), never E[x^2] - E[x]^2; everything above is Chan's pairwise merge.

#define QGN_COLS 64               // columns per workgroup of the moments pass (one per lane)
#define QGN_WAVES 4
#define QGN_MAX_TILES 512         // slab entries per column; the rows per tile grow with n so that this holds
#define QGN_SLICES 16             // the combine pass merges the tiles in 16 runs per column, then a tree over the runs

typedef float qgn_f32x4 __attribute__((ext_vector_type(4)));

// (na, ma, Ma) <- merge with (nb, mb, Mb): Chan et al.  Either side may be empty.
__device__ __forceinline__ void qgn_merge(double &na, double &ma, double &Ma, double nb, double mb, double Mb) {
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
__device__ __forceinline__ void qgn_finish(double cnt, double K, double s1, double s2, double &mean, double &M2) {
    if (cnt == 0.0) {
        mean = 0.0, M2 = 0.0;
        return;
    }
    mean = K + s1 / cnt;
    M2 = fmax(s2 - s1 * s1 / cnt, 0.0);
}

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
        qgn_finish(cnt, K, s1, s2, mean, M2);
        sh[0][t] = cnt, sh[1][t] = mean, sh[2][t] = M2;
        __syncthreads();
        if (wave == 0) {
            for (int w = 1; w < QGN_WAVES; w++) qgn_merge(cnt, mean, M2, sh[0][64 * w + lane], sh[1][64 * w + lane], sh[2][64 * w + lane]);
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
        qgn_finish(cnt, K, s1, s2, mean, M2);
        sh[0][t] = cnt, sh[1][t] = mean, sh[2][t] = M2;
        __syncthreads();
        for (int off = 32 * QGN_WAVES; off >= 1; off >>= 1) {
            if (t < off) {
                qgn_merge(cnt, mean, M2, sh[0][t + off], sh[1][t + off], sh[2][t + off]);
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
        qgn_merge(na, ma, Ma, (double)min(R, n - g * R), p.x, p.y);
    }
    sh[0][t] = na, sh[1][t] = ma, sh[2][t] = Ma;
    __syncthreads();
    for (int off = QGN_SLICES / 2; off >= 1; off >>= 1) {
        if (s < off) {
            qgn_merge(na, ma, Ma, sh[0][t + 16 * off], sh[1][t + 16 * off], sh[2][t + 16 * off]);
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
            const bool d = A.done_kind ? ((const float *)done)[i * A.done_stride] != 0.f : ((const uint8_t *)done)[i * A.done_stride] != 0;
            if (d) returns[i] = 0.0;
        }
    }
}
