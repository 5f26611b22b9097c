// qg_perturb.hip -- sensor noise, sensor bias and actuation latency on rows that are already on the device (include/quadgym.h:
// qg_perturb_*).  An env-step costs TWO launches:
//
//   qg_perturb_actions_kernel   before the env: the action ring takes the policy's row, the servos get the row of d_i env-steps ago
//                               (or reset_action), plus action_std * z.  One thread per (env, joint).
//   qg_perturb_rows_kernel      behind the env (and for an explicit reset): out = in + bias_std[c] * z + obs_std[c] * z per frame
//                               column; advances the env's age and episode.  One wave per env.
//
// Every draw is a pure function of (seed, global env index, episode, stream): nothing random is stored, so a captured launch replays
// with fresh noise (age and episode live in device memory) and shards reproduce the rows of one handle.  No atomics; no workgroup
// reads what another of its launch writes: an env's age and episode are read and written by the one wave that owns the env, which is
// what lets a row be perturbed in place.
//
// Layout of a rows wave.  A normal costs two hashes (ten 64-bit multiplies), logf, sqrtf and cospif, and the kernel is bound by them,
// not by memory: so the lanes are dealt the noisy elements alone.  Lane c < frame_dim forms column c's bias term once; the (slot, noisy
// column) pairs of the row are then taken 64 at a time, each fetching its column's bias term and stds from that column's lane by a
// shuffle.  Columns whose two stds are zero copy their bits (in place: nothing) and never reach the hash: 15 of 26 in a partially
// observable frame, whose 10-frame stack is 110 noisy elements = two passes of a wave.

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>
#include <cstring>

#include "qg_host.h"
#include "qg_key_dev.h"

#define QGP_SALT 0x51474E4F49534531ull
#define QGP_NJ 12
// the handle's constants in device memory (f32): obs_std[64] | bias_std[64] | reset_action[12] | the noisy columns' indices [64]
#define QGP_RESET_ACTION 128
#define QGP_NOISY 140
#define QGP_NCONST 204

// (qgp_mix64, qgp_key, qgp_k -- the keyed draw k(s), on both sides of the launch: qg_key_dev.h)
__host__ __device__ static inline int32_t qgp_delay(uint64_t key, int32_t lo, int32_t hi) {
    return lo + (int32_t)(((uint64_t)qgp_k(key, 0) * (uint64_t)(hi - lo + 1)) >> 24);
}
__host__ __device__ static inline uint64_t qgp_frame_stream(int32_t f, int32_t q) { return 4096ull + 2ull * (128ull * (uint64_t)f + (uint64_t)q); }

// z(s): u1 and 2 * u2 are exact in f32
__device__ __forceinline__ float qgp_normal(uint64_t key, uint64_t stream) {
#pragma clang fp contract(off)
    const float u1 = (float)(qgp_k(key, stream) + 1u) * 0x1p-24f;
    const float two_u2 = (float)qgp_k(key, stream + 1) * 0x1p-23f;
    const float r = sqrtf(-2.0f * logf(u1));
    return r * cospif(two_u2);
}

struct KPerturb {
    int32_t n, F, W, M;            // envs, frame_dim, window, max_delay + 1
    int32_t n_noisy;               // columns with a non-zero std: consts[QGP_NOISY ..] lists them
    int32_t delay_lo, delay_hi;
    int32_t done_row;
    float action_std;
    uint64_t seed_p, base;
};

__global__ __launch_bounds__(256) void qg_perturb_actions_kernel(KPerturb A, const float *actions_in, float *actions_out, float *__restrict__ ring,
                                                                 const int32_t *__restrict__ age, const int64_t *__restrict__ episode,
                                                                 const float *__restrict__ consts) {
#pragma clang fp contract(off)
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;          // n * 12 < 2^31 (qg_perturb_create)
    if (t >= (uint32_t)A.n * QGP_NJ) return;
    const uint32_t i = t / QGP_NJ, j = t - i * QGP_NJ;
    const int32_t a = age[i];
    const uint64_t key = qgp_key(A.seed_p, A.base + i, (uint64_t)episode[i]);
    const int32_t d = A.delay_hi > A.delay_lo ? qgp_delay(key, A.delay_lo, A.delay_hi) : A.delay_lo;
    const float mine = actions_in[t];
    ring[((size_t)(a % A.M) * A.n + i) * QGP_NJ + j] = mine;
    float v = mine;
    if (d > 0) v = a - d >= 0 ? ring[((size_t)((a - d) % A.M) * A.n + i) * QGP_NJ + j] : consts[QGP_RESET_ACTION + j];
    if (A.action_std != 0.f) v = v + A.action_std * qgp_normal(key, qgp_frame_stream(a, 64 + (int32_t)j));
    actions_out[t] = v;
}

// The row of episode `ep` with top frame `top` (quadgym.h).  Every lane of the wave comes here together.  Lane c < frame_dim holds
// column c's two stds and forms its bias term once; the row's work items are the (slot, noisy column) pairs, 64 at a time, and an item
// fetches its column's three values from that column's lane.
__device__ __forceinline__ void qgp_row(const KPerturb &A, const float *src, float *dst, uint64_t env_index, uint64_t ep, int32_t top, int lane,
                                        float ostd_l, float bstd_l, const float *__restrict__ consts) {
#pragma clang fp contract(off)
    const uint64_t key = qgp_key(A.seed_p, env_index, ep);
    const float eb_l = bstd_l != 0.f ? bstd_l * qgp_normal(key, 2u + 2u * (uint32_t)lane) : 0.f;
    const int total = A.W * A.n_noisy;
    for (int base = 0; base < total; base += 64) {               // wave-uniform trip count: the shuffles see every lane
        const int t = base + lane;
        const bool active = t < total;
        const int tt = active ? t : 0;
        const int k = tt / A.n_noisy, c = (int)consts[QGP_NOISY + (tt - k * A.n_noisy)];
        const float eb = __shfl(eb_l, c), ostd = __shfl(ostd_l, c), bstd = __shfl(bstd_l, c);
        if (active) {
            const int32_t f = max(top - (A.W - 1 - k), 0);
            const float x = src[k * A.F + c];
            float e = eb;
            if (ostd != 0.f) {
                const float eo = ostd * qgp_normal(key, qgp_frame_stream(f, c));
                e = bstd != 0.f ? eb + eo : eo;
            }
            dst[k * A.F + c] = x + e;
        }
    }
    if (src != dst)                                              // the quiet columns: their bits
        for (int t = lane; t < A.W * A.F; t += 64) {
            const int c = t % A.F;
            if (consts[c] == 0.f && consts[64 + c] == 0.f) ((uint32_t *)dst)[t] = ((const uint32_t *)src)[t];
        }
}

// BEGIN = false: observe.  BEGIN = true: `done` is the mask (u8, stride 1, nullable: every env), obs_in == obs_out are the rows (nullable)
template <bool BEGIN>
__global__ __launch_bounds__(256) void qg_perturb_rows_kernel(KPerturb A, const float *obs_in, int32_t in_stride, float *obs_out, int32_t out_stride,
                                                              float *terminal, int32_t term_stride, const void *done, int32_t done_kind,
                                                              int32_t done_stride, int32_t *age, int64_t *episode, const float *__restrict__ consts) {
    const int lane = threadIdx.x & 63;
    const int64_t i64 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i64 >= A.n) return;                                      // wave-uniform, as every branch on a, ep, fin below
    const size_t i = (size_t)i64;
    const int32_t a = age[i];
    const uint64_t ep = (uint64_t)episode[i];
    bool fin = BEGIN;
    if (done) {
        if (BEGIN) fin = ((const uint8_t *)done)[i] != 0;
        else fin = qg_done_at(done, done_kind, done_stride, i);
    }
    if (BEGIN && !fin) return;
    const float ostd = consts[lane], bstd = consts[64 + lane];   // zeros from frame_dim on
    const uint64_t env_index = A.base + i;
    if (BEGIN) {
        if (obs_out) qgp_row(A, obs_out + i * out_stride, obs_out + i * out_stride, env_index, ep + 1, 0, lane, ostd, bstd, consts);
    } else if (fin && A.done_row == QG_PERTURB_DONE_ROW_RESET) {
        qgp_row(A, obs_in + i * in_stride, obs_out + i * out_stride, env_index, ep + 1, 0, lane, ostd, bstd, consts);
        if (terminal) qgp_row(A, terminal + i * term_stride, terminal + i * term_stride, env_index, ep, a + 1, lane, ostd, bstd, consts);
    } else {
        qgp_row(A, obs_in + i * in_stride, obs_out + i * out_stride, env_index, ep, a + 1, lane, ostd, bstd, consts);
    }
    if (lane == 0) {                                             // (every lane's loads of the two words precede this store in program order)
        age[i] = fin ? 0 : a + 1;
        if (fin) episode[i] = (int64_t)(ep + 1);
    }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
struct qg_perturb {
    int32_t device;
    qg_perturb_desc desc;
    KPerturb k;
    QgDevMem mem;
    int32_t *d_age;           // [n]
    int64_t *d_episode;       // [n]
    float *d_ring;            // [max_delay + 1][n][12]
    float *d_consts;          // [QGP_NCONST]
};

static int perturb_validate(const qg_perturb_desc *d) {
    if (!d) return fail(QG_ERR_ARG, "qg_perturb: null description");
    QG_CHECK_STRUCT(d, qg_perturb_desc);
    if (d->n_envs < 1 || (int64_t)d->n_envs * QGP_NJ * (QG_PERTURB_MAX_DELAY + 1) > INT32_MAX)
        return fail(QG_ERR_ARG, "qg_perturb: n_envs %d outside 1 .. %d", d->n_envs, INT32_MAX / (QGP_NJ * (QG_PERTURB_MAX_DELAY + 1)));
    if (d->frame_dim < 1 || d->frame_dim > 64) return fail(QG_ERR_ARG, "qg_perturb: frame_dim %d outside 1 .. 64", d->frame_dim);
    if (d->window < 1 || d->window > 64) return fail(QG_ERR_ARG, "qg_perturb: window %d outside 1 .. 64", d->window);
    if (d->max_delay < 0 || d->max_delay > QG_PERTURB_MAX_DELAY)
        return fail(QG_ERR_ARG, "qg_perturb: max_delay %d outside 0 .. %d", d->max_delay, QG_PERTURB_MAX_DELAY);
    if (d->delay_lo < 0 || d->delay_lo > d->delay_hi || d->delay_hi > d->max_delay)
        return fail(QG_ERR_ARG, "qg_perturb: delays (%d, %d) must satisfy 0 <= delay_lo <= delay_hi <= max_delay = %d", d->delay_lo, d->delay_hi,
                    d->max_delay);
    if (d->done_row != QG_PERTURB_DONE_ROW_RESET && d->done_row != QG_PERTURB_DONE_ROW_TERMINAL)
        return fail(QG_ERR_ARG, "qg_perturb: done_row %d is neither QG_PERTURB_DONE_ROW_RESET nor _TERMINAL", d->done_row);
    if (d->reserved != 0) return fail(QG_ERR_ARG, "qg_perturb: reserved must be 0");
    if (!qg_finite32(d->action_std) || d->action_std < 0.f) return fail(QG_ERR_ARG, "qg_perturb: action_std %g must be finite and >= 0", d->action_std);
    for (int c = 0; c < 64; c++)
        if (!qg_finite32(d->obs_std[c]) || d->obs_std[c] < 0.f || !qg_finite32(d->bias_std[c]) || d->bias_std[c] < 0.f)
            return fail(QG_ERR_ARG, "qg_perturb: column %d: obs_std %g, bias_std %g must be finite and >= 0", c, d->obs_std[c], d->bias_std[c]);
    for (int j = 0; j < QGP_NJ; j++)
        if (!qg_finite32(d->reset_action[j])) return fail(QG_ERR_ARG, "qg_perturb: reset_action[%d] is not finite", j);
    return QG_OK;
}

extern "C" int qg_perturb_destroy(qg_perturb *p) {
    if (p) qg_free_handle(p, p->device);           // launches may still be in flight on a caller's stream
    return QG_OK;
}

extern "C" int qg_perturb_create(int32_t device_id, const qg_perturb_desc *desc, qg_perturb **out) {
    if (!out) return fail(QG_ERR_ARG, "qg_perturb_create: null output");
    *out = nullptr;
    QG_TRY(perturb_validate(desc));
    QG_TRY(qg_open_device(device_id, nullptr));
    qg_perturb *p = qg_new_handle<qg_perturb>();
    if (!p) return QG_ERR_ALLOC;
    p->device = device_id;
    p->desc = *desc;
    KPerturb &k = p->k;
    k.n = desc->n_envs, k.F = desc->frame_dim, k.W = desc->window, k.M = desc->max_delay + 1;
    k.delay_lo = desc->delay_lo, k.delay_hi = desc->delay_hi, k.done_row = desc->done_row;
    k.action_std = desc->action_std;
    k.seed_p = desc->seed + QGP_SALT, k.base = desc->env_index_base;
    const size_t n = (size_t)k.n;
    if (p->mem.alloc(p->d_age, n * sizeof(int32_t), true) || p->mem.alloc(p->d_episode, n * sizeof(int64_t), true) ||
        p->mem.alloc(p->d_ring, (size_t)k.M * n * QGP_NJ * sizeof(float), true) || p->mem.alloc(p->d_consts, QGP_NCONST * sizeof(float))) {
        qg_perturb_destroy(p);
        return QG_ERR_ALLOC;
    }
    float stds[QGP_NCONST] = {0};
    memcpy(stds + QGP_RESET_ACTION, desc->reset_action, sizeof desc->reset_action);
    for (int c = 0; c < 64; c++) stds[c] = c < k.F ? desc->obs_std[c] : 0.f, stds[64 + c] = c < k.F ? desc->bias_std[c] : 0.f;
    for (int c = 0; c < k.F; c++)
        if (stds[c] != 0.f || stds[64 + c] != 0.f) stds[QGP_NOISY + k.n_noisy++] = (float)c;
    hipError_t e = hipMemcpy(p->d_consts, stds, sizeof stds, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        qg_perturb_destroy(p);
        return fail(QG_ERR_DEVICE, "qg_perturb_create: %s", hipGetErrorString(e));
    }
    *out = p;
    return QG_OK;
}

extern "C" int qg_perturb_actions_device(qg_perturb *p, int32_t n, const float *actions_in, float *actions_out, void *stream) {
    if (!p || !actions_in || !actions_out) return fail(QG_ERR_ARG, "qg_perturb_actions_device: null argument");
    if (n != p->desc.n_envs) return fail(QG_ERR_ARG, "qg_perturb_actions_device: n is %d, the handle was built for %d envs", n, p->desc.n_envs);
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    const unsigned blocks = (unsigned)(((int64_t)n * QGP_NJ + 255) / 256);
    qg_perturb_actions_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(p->k, actions_in, actions_out, p->d_ring, p->d_age, p->d_episode, p->d_consts);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_perturb_observe_device(qg_perturb *p, int32_t n, const float *obs_in, int32_t in_stride, float *obs_out, int32_t out_stride,
                                         float *terminal_obs, int32_t terminal_stride, const void *done, int32_t done_kind, int32_t done_stride,
                                         void *stream) {
    if (!p || !obs_in || !obs_out) return fail(QG_ERR_ARG, "qg_perturb_observe_device: null argument");
    if (n != p->desc.n_envs) return fail(QG_ERR_ARG, "qg_perturb_observe_device: n is %d, the handle was built for %d envs", n, p->desc.n_envs);
    const int32_t row = p->k.F * p->k.W;
    if (in_stride < row || out_stride < row)
        return fail(QG_ERR_ARG, "qg_perturb_observe_device: strides %d, %d < window * frame_dim = %d", in_stride, out_stride, row);
    if (terminal_obs) {
        if (p->desc.done_row != QG_PERTURB_DONE_ROW_RESET)
            return fail(QG_ERR_ARG, "qg_perturb_observe_device: terminal_obs goes with QG_PERTURB_DONE_ROW_RESET (the row is the terminal observation)");
        if (terminal_stride < row) return fail(QG_ERR_ARG, "qg_perturb_observe_device: terminal_stride %d < window * frame_dim = %d", terminal_stride, row);
    }
    QG_TRY(qg_check_done("qg_perturb_observe_device", done, done_kind, done_stride));
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    qg_perturb_rows_kernel<false><<<(unsigned)((n + 3) / 4), 256, 0, (hipStream_t)stream>>>(p->k, obs_in, in_stride, obs_out, out_stride, terminal_obs,
                                                                                          terminal_stride, done, done_kind, done_stride, p->d_age,
                                                                                          p->d_episode, p->d_consts);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_perturb_begin_device(qg_perturb *p, int32_t n, const uint8_t *mask, float *rows, int32_t row_stride, void *stream) {
    if (!p) return fail(QG_ERR_ARG, "qg_perturb_begin_device: null argument");
    if (n != p->desc.n_envs) return fail(QG_ERR_ARG, "qg_perturb_begin_device: n is %d, the handle was built for %d envs", n, p->desc.n_envs);
    if (rows && row_stride < p->k.F * p->k.W)
        return fail(QG_ERR_ARG, "qg_perturb_begin_device: row_stride %d < window * frame_dim = %d", row_stride, p->k.F * p->k.W);
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    qg_perturb_rows_kernel<true><<<(unsigned)((n + 3) / 4), 256, 0, (hipStream_t)stream>>>(p->k, rows, row_stride, rows, row_stride, nullptr, 0, mask,
                                                                                         QG_DONE_U8, 1, p->d_age, p->d_episode, p->d_consts);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_perturb_get_delays(qg_perturb *p, int32_t *delays) {
    if (!p || !delays) return fail(QG_ERR_ARG, "qg_perturb_get_delays: null argument");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    const size_t n = (size_t)p->k.n;
    QgHostBuf<int64_t> ep(n);
    QG_TRY(ep.oom());
    HIP_TRY(hipMemcpy(ep, p->d_episode, n * sizeof(int64_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    for (size_t i = 0; i < n; i++) delays[i] = qgp_delay(qgp_key(p->k.seed_p, p->k.base + i, (uint64_t)ep[i]), p->k.delay_lo, p->k.delay_hi);
    return QG_OK;
}

extern "C" int qg_perturb_get_state(qg_perturb *p, int32_t *age, int64_t *episode, float *ring) {
    if (!p || !age || !episode || !ring) return fail(QG_ERR_ARG, "qg_perturb_get_state: null argument");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);         // a launch may be in flight on a caller's stream
    const size_t n = (size_t)p->k.n;
    HIP_TRY(hipMemcpy(age, p->d_age, n * sizeof(int32_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(episode, p->d_episode, n * sizeof(int64_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(ring, p->d_ring, (size_t)p->k.M * n * QGP_NJ * sizeof(float), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    return QG_OK;
}

extern "C" int qg_perturb_set_state(qg_perturb *p, const int32_t *age, const int64_t *episode, const float *ring) {
    if (!p || !age || !episode || !ring) return fail(QG_ERR_ARG, "qg_perturb_set_state: null argument");
    const size_t n = (size_t)p->k.n;
    for (size_t i = 0; i < n; i++)
        if (age[i] < 0 || age[i] >= (1 << 23) || episode[i] < 0 || episode[i] >= ((int64_t)1 << 62))
            return fail(QG_ERR_ARG, "qg_perturb_set_state: env %zu: age %d (0 .. 2^23 - 1), episode %lld (0 .. 2^62 - 1)", i, age[i],
                        (long long)episode[i]);
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    HIP_TRY(hipMemcpy(p->d_age, age, n * sizeof(int32_t), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(p->d_episode, episode, n * sizeof(int64_t), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(p->d_ring, ring, (size_t)p->k.M * n * QGP_NJ * sizeof(float), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    return QG_OK;
}
