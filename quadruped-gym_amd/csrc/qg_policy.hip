// qg_policy.hip -- the fused MLP policy forward pass (include/quadgym.h: qg_policy_*): actor tower, optional critic tower and the
// diagonal-Gaussian epilogue in ONE launch, exact f32 on the f32-input matrix instruction (v_mfma_f32_16x16x4_f32).
//
// Layout.  A workgroup owns a tile of 16 envs and one tower (blockIdx.y).  Every layer computes H^T = W . X^T: the 16
// envs sit on the matrix instruction's column (lane & 15), output features on its rows, so lane (g = lane >> 4, e = lane & 15) holds
// features 16m + 4g + {0..3} of env e in the four accumulator registers of output block m.  Those four registers are, unchanged, the
// B operands of the next layer's k-steps 4m .. 4m + 3 when k-step s of a 16-feature block takes feature 4g + s from lane group g:
// the A operand of that k-step is then W[row][16q + 4g + s], four consecutive floats of a row of W per lane and block of 16 inputs.
// Activations pass from layer to layer through LDS in that very register image ([16-feature block][lane] float4: one ds_write_b128 per
// accumulator, one conflict-free ds_read_b128 per four k-steps), so the output blocks of a layer can be shared out over the waves
// of the workgroup; nothing between the observation row and the outputs touches global memory.
//
// Weights are read from the packed image qg_policy_pack_kernel writes ([layer][output block][block of 16 inputs][lane] float4, zero
// padded: a wave's load is 1 KiB contiguous), two chunks of 16 float4 per lane in flight ahead of the matrix instructions.
//
// Numerics: every output is a k-ordered fmaf chain that starts from the bias, in a fixed order that depends on nothing but the
// layer sizes -- a row's results do not depend on n, on its place in the tile or on the other rows.

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>
#include <cstring>
#include <new>

#include "qg_policy.h"

// canonical flat parameters -> the packed image (one thread per packed float; runs on the caller's stream after every update)
__global__ void qg_policy_pack_kernel(KPolicy P, const float *__restrict__ src, float *__restrict__ packed) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.packed_floats) return;
    if (i >= P.std_off) {
        const int a = (i - P.std_off) & 15;
        const bool is_std = i - P.std_off < 16;
        float v = 0.f;
        if (a < P.act_dim) {
            const float ls = src[P.src_log_std + a];
            v = is_std ? (float)exp((double)ls) : ls;      // exp in f64, rounded once: the correctly rounded f32 standard deviation
        }
        packed[i] = v;
        return;
    }
    for (int t = 0; t < P.n_towers; t++)
        for (int l = 0; l < P.n_layers; l++) {
            const KPolLayer L = P.layer[t][l];
            const int wn = L.nb * L.nq * 256;
            if (i >= L.w_off && i < L.w_off + wn) {
                const int j = i - L.w_off;
                const int s = j & 3, lane = (j >> 2) & 63, rest = j >> 8;
                const int q = rest % L.nq, m = rest / L.nq;
                const int row = 16 * m + (lane & 15), col = 16 * q + 4 * (lane >> 4) + s;
                packed[i] = (row < L.out_dim && col < L.in_dim) ? src[L.src_w + row * L.in_dim + col] : 0.f;
                return;
            }
            if (i >= L.b_off && i < L.b_off + 16 * L.nb) {
                const int row = i - L.b_off;
                packed[i] = row < L.out_dim ? src[L.src_b + row] : 0.f;
                return;
            }
        }
}

// one chunk of A operands: KQ blocks of 16 inputs for each of the wave's MB output blocks (m = wave + WAVES * i).  Indices past the
// layer's end are clamped, not branched around (a branch per load would serialise them); the matrix instructions are what is guarded,
// per block of 16 inputs.
template <int WAVES, int MB, int KQ>
__device__ __forceinline__ void qgp_load_chunk(qgp_f32x4 (&w)[MB][KQ], const float *__restrict__ packed, const KPolLayer &L, int q0, int wave,
                                               int lane) {
    const qgp_f32x4 *wp = (const qgp_f32x4 *)(packed + L.w_off);
#pragma unroll
    for (int i = 0; i < MB; i++) {
        const int m = min(wave + WAVES * i, L.nb - 1);
#pragma unroll
        for (int kq = 0; kq < KQ; kq++) {
            const int q = min(q0 + kq, L.nq - 1);
            w[i][kq] = wp[(m * L.nq + q) * 64 + lane];
        }
    }
}

// the matrix instructions of one chunk on the first NB accumulators (s outer, block inner: consecutive instructions are independent;
// each accumulator still takes its products in ascending k)
template <int MB, int KQ, int NB>
__device__ __forceinline__ void qgp_mfma_chunk(qgp_f32x4 (&acc)[MB], const qgp_f32x4 (&w)[MB][KQ], const qgp_f32x4 *xin, int nq, int q0, int lane) {
#pragma unroll
    for (int kq = 0; kq < KQ; kq++) {
        const int q = q0 + kq;
        if (q < nq) {
            const qgp_f32x4 b = xin[q * 64 + lane];
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int i = 0; i < NB; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[i][kq][s], b[s], acc[i], 0, 0, 0);
        }
    }
}

// A wave with one output block in this layer (the output layer; the last blocks of a layer that does not fill every wave) runs one
// accumulator; with more it runs all MB -- accumulators past the wave's last block chew on clamped weights and are never stored.
template <int MB, int KQ>
__device__ __forceinline__ void qgp_mfma_blocks(qgp_f32x4 (&acc)[MB], const qgp_f32x4 (&w)[MB][KQ], const qgp_f32x4 *xin, int nq, int nbw, int q0,
                                                int lane) {
    if (nbw > 1) qgp_mfma_chunk<MB, KQ, MB>(acc, w, xin, nq, q0, lane);
    else if (nbw == 1) qgp_mfma_chunk<MB, KQ, 1>(acc, w, xin, nq, q0, lane);
}

// mean + std * eps with the product rounded before the sum (no contraction into an fma): the two roundings the formula reads with
__device__ __forceinline__ float qgp_sample(float mean, float std, float eps) {
#pragma clang fp contract(off)
    const float prod = std * eps;
    return mean + prod;
}

template <int WAVES, int MB>
__global__ __launch_bounds__(64 * WAVES) void qg_policy_forward_kernel(KPolicy P, const float *__restrict__ packed, int n,
                                                                       const float *__restrict__ obs, int obs_stride,
                                                                       const float *__restrict__ eps, float *__restrict__ actions,
                                                                       float *__restrict__ log_prob, float *__restrict__ value) {
    constexpr int KQ = 16 / MB;
    extern __shared__ qgp_f32x4 qgp_lds[];
    const int tower = blockIdx.y, env0 = blockIdx.x * QGP_TILE;
    const int lane = threadIdx.x & 63, e = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // wave-uniform, and known to be: what depends on it branches, not masks
    float *x0 = (float *)qgp_lds;
    float *x1 = x0 + P.lds0_floats;

    qgp_f32x4 wa[MB][KQ], wb[MB][KQ];
    qgp_load_chunk<WAVES, MB, KQ>(wa, packed, P.layer[tower][0], 0, wave, lane);

    // the observation tile into buffer 0 in the operand image: feature c of env ee at float ((c >> 2) * 16 + ee) * 4 + (c & 3).  A wave
    // takes rows wave, wave + WAVES, ..; a lane the columns lane, lane + 64, ..  Every load of a batch (16 per lane) is issued before
    // the first LDS write, so the tile costs a few global-memory latencies, not one per row; addresses past the row or the batch are
    // clamped and the value dropped.
    {
        constexpr int R = QGP_TILE / WAVES;
        constexpr int JU = WAVES == 1 ? 1 : 4;
        const int width = 16 * P.layer[tower][0].nq;
        // the tower's window of the row (wave-uniform): the actor's columns [0, obs_dim), the critic's [critic_off, .. + its input width)
        const int in_dim = tower ? P.layer[1][0].in_dim : P.obs_dim, in_off = tower ? P.critic_off : 0;
        for (int c0 = lane; c0 < width + lane; c0 += 64 * JU) {
            float v[JU][R];
#pragma unroll
            for (int ju = 0; ju < JU; ju++)
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int env = env0 + wave + WAVES * r;
                    v[ju][r] = obs[(size_t)min(env, n - 1) * obs_stride + in_off + min(c0 + 64 * ju, in_dim - 1)];
                }
#pragma unroll
            for (int ju = 0; ju < JU; ju++)
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const int c = c0 + 64 * ju, ee = wave + WAVES * r;
                    if (c < width) x0[((c >> 2) * 16 + ee) * 4 + (c & 3)] = (c < in_dim && env0 + ee < n) ? v[ju][r] : 0.f;
                }
        }
    }

    for (int l = 0; l < P.n_layers; l++) {
        const KPolLayer L = P.layer[tower][l];
        const bool last = l == P.n_layers - 1;
        const KPolLayer LN = P.layer[tower][last ? l : l + 1];
        const qgp_f32x4 *xin = (const qgp_f32x4 *)((l & 1) ? x1 : x0);
        qgp_f32x4 *xout = (qgp_f32x4 *)((l & 1) ? x0 : x1);
        const int nbw = L.nb > wave ? (L.nb - wave + WAVES - 1) / WAVES : 0;      // output blocks of this wave

        qgp_f32x4 acc[MB];
#pragma unroll
        for (int i = 0; i < MB; i++) {
            const int m = min(wave + WAVES * i, L.nb - 1);
            acc[i] = *(const qgp_f32x4 *)(packed + L.b_off + 16 * m + 4 * g);
        }
        __syncthreads();          // the layer's input is complete (and the buffer it overwrites has been read by every wave)

        for (int q0 = 0; q0 < L.nq; q0 += 2 * KQ) {
            qgp_load_chunk<WAVES, MB, KQ>(wb, packed, L, q0 + KQ, wave, lane);
            qgp_mfma_blocks<MB, KQ>(acc, wa, xin, L.nq, nbw, q0, lane);
            // the chunk after next: this layer's, or the first of the next layer (its latency hides behind the epilogue and the barrier)
            const bool more = q0 + 2 * KQ < L.nq;
            qgp_load_chunk<WAVES, MB, KQ>(wa, packed, more ? L : LN, more ? q0 + 2 * KQ : 0, wave, lane);
            qgp_mfma_blocks<MB, KQ>(acc, wb, xin, L.nq, nbw, q0 + KQ, lane);
        }

        if (!last) {
#pragma unroll
            for (int i = 0; i < MB; i++)
                if (i < nbw) {
                    qgp_f32x4 h;
#pragma unroll
                    for (int r = 0; r < 4; r++) h[r] = tanhf(acc[i][r]);
                    xout[(wave + WAVES * i) * 64 + lane] = h;
                }
        } else if (wave == 0) {
            const int env = env0 + e;
            const bool live = env < n;
            if (tower == 1) {
                if (value && g == 0 && live) value[env] = acc[0][0];
            } else {
                const float *sd = packed + P.std_off;
                double lp = 0.0;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int a = 4 * g + r;
                    if (a < P.act_dim) {
                        float mean = acc[0][r];
                        if (P.out_tanh) mean = tanhf(mean);
                        float act = mean, ev = 0.f;
                        if (eps) {
                            ev = live ? eps[(size_t)env * P.act_dim + a] : 0.f;
                            act = qgp_sample(mean, sd[a], ev);
                        }
                        if (live) actions[(size_t)env * P.act_dim + a] = act;
                        lp += -0.5 * (double)ev * (double)ev - (double)sd[16 + a] - QGG_HALF_LOG_2PI;
                    }
                }
                if (log_prob) {   // the sum over the action components runs over the four lane groups (f64: rounded to f32 once)
                    lp += __shfl_xor(lp, 16);
                    lp += __shfl_xor(lp, 32);
                    if (g == 0 && live) log_prob[env] = (float)lp;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
// the description is valid: fills the kernel's layer table (offsets into both parameter images) and returns the canonical length.
// critic_dim < 0: the critic reads the actor's columns (qg_policy_create); else its window (qg_policy_create_asym)
static int policy_layout(const qg_policy_desc *d, KPolicy *k, int32_t critic_off = 0, int32_t critic_dim = -1) {
    if (!d) return fail(QG_ERR_ARG, "qg_policy: null description");
    QG_CHECK_STRUCT(d, qg_policy_desc);
    if (d->obs_dim < 1 || d->obs_dim > 512) return fail(QG_ERR_ARG, "qg_policy: obs_dim %d outside 1 .. 512", d->obs_dim);
    if (d->act_dim < 1 || d->act_dim > 16) return fail(QG_ERR_ARG, "qg_policy: act_dim %d outside 1 .. 16", d->act_dim);
    if (d->n_hidden < 1 || d->n_hidden > 3) return fail(QG_ERR_ARG, "qg_policy: n_hidden %d outside 1 .. 3", d->n_hidden);
    for (int i = 0; i < d->n_hidden; i++)
        if (d->hidden[i] < 16 || d->hidden[i] > 256 || d->hidden[i] % 16)
            return fail(QG_ERR_ARG, "qg_policy: hidden[%d] = %d (a multiple of 16, 16 .. 256; tanh layers only)", i, d->hidden[i]);
    if ((d->out_tanh != 0 && d->out_tanh != 1) || (d->has_value != 0 && d->has_value != 1))
        return fail(QG_ERR_ARG, "qg_policy: out_tanh and has_value are 0 or 1");
    if (critic_dim >= 0) {
        if (!d->has_value) return fail(QG_ERR_ARG, "qg_policy: a critic window, but has_value is 0");
        if (critic_dim < 1 || critic_dim > 512) return fail(QG_ERR_ARG, "qg_policy: critic_obs_dim %d outside 1 .. 512", critic_dim);
        if (critic_off < 0 || critic_off > 512 - critic_dim)
            return fail(QG_ERR_ARG, "qg_policy: critic_obs_offset %d: the window must lie in columns 0 .. 512 (offset + dim = %lld)", critic_off,
                        (long long)critic_off + critic_dim);
    } else {
        critic_off = 0, critic_dim = d->obs_dim;
    }
    KPolicy p;
    memset(&p, 0, sizeof p);
    p.obs_dim = d->obs_dim;
    p.critic_off = critic_off;
    p.act_dim = d->act_dim;
    p.n_layers = d->n_hidden + 1;
    p.out_tanh = d->out_tanh;
    p.n_towers = d->has_value ? 2 : 1;
    int src = 0, dst = 0;
    for (int t = 0; t < p.n_towers; t++) {
        int in = t == 0 ? d->obs_dim : critic_dim;
        for (int l = 0; l < p.n_layers; l++) {
            const int out = l < d->n_hidden ? d->hidden[l] : (t == 0 ? d->act_dim : 1);
            KPolLayer &L = p.layer[t][l];
            L.in_dim = in;
            L.out_dim = out;
            L.nq = (in + 15) / 16;
            L.nb = (out + 15) / 16;
            L.src_w = src;
            L.src_b = src + out * in;
            src += out * in + out;
            L.w_off = dst;
            L.b_off = dst + L.nb * L.nq * 256;
            dst = L.b_off + 16 * L.nb;
            in = out;
        }
        if (t == 0) {
            p.src_log_std = src;
            src += d->act_dim;
        }
    }
    p.std_off = dst;
    p.packed_floats = dst + 32;
    // activation buffers, floats (16 envs per feature): layer l reads buffer l & 1 and writes the other
    int f0 = 16 * p.layer[0][0].nq, f1 = d->hidden[0];
    if (p.n_towers == 2 && 16 * p.layer[1][0].nq > f0) f0 = 16 * p.layer[1][0].nq;      // the wider of the two towers' first layers
    if (d->n_hidden > 1 && d->hidden[1] > f0) f0 = d->hidden[1];
    if (d->n_hidden > 2 && d->hidden[2] > f1) f1 = d->hidden[2];
    p.lds0_floats = 16 * f0;
    p.lds1_floats = 16 * f1;
    if (k) *k = p;
    return src;
}

extern "C" int qg_policy_param_count(const qg_policy_desc *desc) { return policy_layout(desc, nullptr); }
extern "C" int qg_policy_param_count_asym(const qg_policy_desc *desc, int32_t critic_obs_dim) {
    if (critic_obs_dim < 0) return fail(QG_ERR_ARG, "qg_policy: critic_obs_dim %d outside 1 .. 512", critic_obs_dim);
    return policy_layout(desc, nullptr, 0, critic_obs_dim);
}

extern "C" int qg_policy_destroy(qg_policy *p) {
    if (p) qg_free_handle(p, p->device);           // forward passes may still be in flight on a caller's stream
    return QG_OK;
}

static int policy_pack(qg_policy *p, hipStream_t st) {
    const int threads = 256;
    qg_policy_pack_kernel<<<(p->k.packed_floats + threads - 1) / threads, threads, 0, st>>>(p->k, p->d_params, p->d_packed);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return qg_policy_pack_transposed(p, st);       // the gradient pass's image, once qg_policy_reserve_grad has been called
}

static int policy_create(int32_t device_id, const qg_policy_desc *desc, int32_t critic_off, int32_t critic_dim, qg_policy **out) {
    if (!out) return fail(QG_ERR_ARG, "qg_policy_create: null output");
    *out = nullptr;
    KPolicy k;
    const int count = policy_layout(desc, &k, critic_off, critic_dim);
    if (count < 0) return count;
    int simds;
    QG_TRY(qg_open_device(device_id, &simds));
    qg_policy *p = qg_new_handle<qg_policy>();
    if (!p) return QG_ERR_ALLOC;
    p->device = device_id;
    p->desc = *desc;
    p->k = k;
    p->n_params = count;
    p->simds = simds;
    if (const char *e = getenv("QG_POLICY_WAVES")) p->force_waves = atoi(e) == 1 ? 1 : (atoi(e) == 4 ? 4 : 0);
    if (p->mem.alloc(p->d_params, (size_t)count * sizeof(float), true) || p->mem.alloc(p->d_packed, (size_t)k.packed_floats * sizeof(float))) {
        qg_policy_destroy(p);
        return QG_ERR_ALLOC;
    }
    int rc = policy_pack(p, nullptr);
    if (rc == QG_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(QG_ERR_LAUNCH, "qg_policy_create: the packing launch failed");
    if (rc != QG_OK) {
        qg_policy_destroy(p);
        return rc;
    }
    *out = p;
    return QG_OK;
}

extern "C" int qg_policy_create(int32_t device_id, const qg_policy_desc *desc, qg_policy **out) {
    return policy_create(device_id, desc, 0, -1, out);
}

extern "C" int qg_policy_create_asym(int32_t device_id, const qg_policy_desc *desc, int32_t critic_obs_offset, int32_t critic_obs_dim,
                                     qg_policy **out) {
    if (critic_obs_dim < 0) {
        if (out) *out = nullptr;
        return fail(QG_ERR_ARG, "qg_policy: critic_obs_dim %d outside 1 .. 512", critic_obs_dim);
    }
    return policy_create(device_id, desc, critic_obs_offset, critic_obs_dim, out);
}

extern "C" int qg_policy_critic_window(const qg_policy *p, int32_t *offset, int32_t *dim) {
    if (!p || !offset || !dim) return fail(QG_ERR_ARG, "qg_policy_critic_window: null argument");
    *offset = p->k.critic_off;
    *dim = p->k.n_towers == 2 ? p->k.layer[1][0].in_dim : p->desc.obs_dim;
    return QG_OK;
}

extern "C" int qg_policy_set_params(qg_policy *p, const float *host_params) {
    if (!p || !host_params) return fail(QG_ERR_ARG, "qg_policy_set_params: null argument");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);         // forward passes on a caller's stream read the image this rewrites
    HIP_TRY(hipMemcpy(p->d_params, host_params, (size_t)p->n_params * sizeof(float), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    QG_TRY(policy_pack(p, nullptr));
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_policy_get_params(qg_policy *p, float *host_params) {
    if (!p || !host_params) return fail(QG_ERR_ARG, "qg_policy_get_params: null argument");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);         // an update may be in flight on a caller's stream
    HIP_TRY(hipMemcpy(host_params, p->d_params, (size_t)p->n_params * sizeof(float), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    return QG_OK;
}

extern "C" int qg_policy_set_params_device(qg_policy *p, const float *d_params, void *stream) {
    if (!p || !d_params) return fail(QG_ERR_ARG, "qg_policy_set_params_device: null argument");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    const hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(p->d_params, d_params, (size_t)p->n_params * sizeof(float), hipMemcpyDeviceToDevice, st), QG_ERR_LAUNCH);
    return policy_pack(p, st);
}

template <int WAVES, int MB>
static void launch_policy(const qg_policy *p, int32_t n, const float *obs, int32_t obs_stride, const float *eps, float *actions,
                          float *log_prob, float *value, hipStream_t st) {
    const dim3 grid((unsigned)((n + QGP_TILE - 1) / QGP_TILE), value ? (unsigned)p->k.n_towers : 1u);
    const size_t lds = (size_t)(p->k.lds0_floats + p->k.lds1_floats) * sizeof(float);
    qg_policy_forward_kernel<WAVES, MB><<<grid, 64 * WAVES, lds, st>>>(p->k, p->d_packed, n, obs, obs_stride, eps, actions, log_prob, value);
}

// Waves per 16-env tile and output blocks per wave: four waves -- the output blocks of a layer shared out, one barrier per
// layer -- for nets wider than 64 at every size, and for the narrow ones while one wave per tile would leave SIMDs without a wave; one
// from there on.  A wave holds the blocks of a 64-wide layer (1 on four waves, 4 on one) or of a 256-wide one (4, 16).
static void policy_launch_shape(const qg_policy *p, int32_t n, bool with_value, int32_t *waves, int32_t *blocks) {
    int widest = 0;
    for (int i = 0; i < p->desc.n_hidden; i++) widest = p->desc.hidden[i] > widest ? p->desc.hidden[i] : widest;
    const int towers = with_value ? p->k.n_towers : 1;     // no value buffer: the critic tower is not launched
    const int64_t tiles = ((int64_t)(n + QGP_TILE - 1) / QGP_TILE) * towers;
    *waves = p->force_waves ? p->force_waves : ((widest > 64 || tiles < (int64_t)p->simds) ? 4 : 1);
    *blocks = *waves == 4 ? (widest <= 64 ? 1 : 4) : (widest <= 64 ? 4 : 16);
}

extern "C" int qg_policy_launch_shape(const qg_policy *p, int32_t n, int32_t with_value, int32_t *waves, int32_t *blocks) {
    if (!p || !waves || !blocks) return fail(QG_ERR_ARG, "qg_policy_launch_shape: null argument");
    if (n < 1) return fail(QG_ERR_ARG, "qg_policy_launch_shape: n must be >= 1");
    if (with_value && !p->desc.has_value) return fail(QG_ERR_ARG, "qg_policy_launch_shape: with_value, but the policy has no critic tower");
    policy_launch_shape(p, n, with_value != 0, waves, blocks);
    return QG_OK;
}

extern "C" int qg_policy_forward_device(qg_policy *p, int32_t n, const float *obs, int32_t obs_stride, const float *eps, float *actions,
                                        float *log_prob, float *value, void *stream) {
    if (!p || !obs || !actions) return fail(QG_ERR_ARG, "qg_policy_forward_device: null argument");
    if (n < 1) return fail(QG_ERR_ARG, "qg_policy_forward_device: n must be >= 1");
    if (obs_stride < p->desc.obs_dim) return fail(QG_ERR_ARG, "qg_policy_forward_device: obs_stride %d < obs_dim %d", obs_stride, p->desc.obs_dim);
    if (value && !p->desc.has_value) return fail(QG_ERR_ARG, "qg_policy_forward_device: a value buffer, but the policy has no critic tower");
    if (obs_stride < qg_policy_row_width(p, value != nullptr))
        return fail(QG_ERR_ARG, "qg_policy_forward_device: obs_stride %d < %d, the end of the critic's window", obs_stride, qg_policy_row_width(p, true));
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    const hipStream_t st = (hipStream_t)stream;
    int32_t waves, blocks;
    policy_launch_shape(p, n, value != nullptr, &waves, &blocks);
    if (waves == 4 && blocks == 1) launch_policy<4, 1>(p, n, obs, obs_stride, eps, actions, log_prob, value, st);
    else if (waves == 4 && blocks == 4) launch_policy<4, 4>(p, n, obs, obs_stride, eps, actions, log_prob, value, st);
    else if (waves == 1 && blocks == 4) launch_policy<1, 4>(p, n, obs, obs_stride, eps, actions, log_prob, value, st);
    else if (waves == 1 && blocks == 16) launch_policy<1, 16>(p, n, obs, obs_stride, eps, actions, log_prob, value, st);
    // only if policy_launch_shape and the launch sites above drift apart (tests/test_policy_api.py compares them on the host)
    else return fail(QG_ERR_LAUNCH, "qg_policy_forward_device: no kernel for %d waves x %d blocks", waves, blocks);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}
