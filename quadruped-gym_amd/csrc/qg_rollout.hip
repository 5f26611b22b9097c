// qg_rollout.hip -- the PPO rollout buffer on the device (include/quadgym.h: qg_rollout_*): SB3's RolloutBuffer over tensors the caller
// owns, filled by launches that a hipGraph can replay.  Four kernels, one launch per entry point:
//
//   qg_rollout_begin_kernel    cursor = 0; slot 0 of obs takes the caller's rows, or the slot the cursor stood on
//   qg_rollout_add_kernel      the record of one env-step into slot `cursor`, the next observation into slot cursor + 1, the per-env
//                              episode accumulators, cursor + 1
//   qg_rollout_gae_kernel      advantages and returns of the filled slots: one lane per env walks time backwards
//   qg_rollout_gather_kernel   rows idx[b] of the filled slots into a minibatch
//
// The cursor lives in device memory (QgrCtl).  A launch that moves it reads it once per workgroup -- lane 0, then through LDS -- and
// only then takes an integer ticket; the workgroup that draws the last ticket of the grid (through two levels of counters) writes
// the new cursor.  Every read of the cursor in a launch therefore precedes that launch's write of it: no workgroup sees the cursor
// its own launch writes, and the next launch sees it through the kernel boundary.  Nothing else passes between the workgroups of a
// launch.
//
// No floating-point atomics; the integer ones are the ticket and the two error counters.  Every stored float depends on its own env
// or sample alone, so the results do not depend on the launch shape.
//
// Layout.  Row copies run lanes along the columns of a row (16 bytes per lane where the row length, the strides and the bases allow
// it, 4 bytes otherwise: the rule of qg_norm).  The per-env work -- the scalars of a step, the episode accumulators, the whole GAE
// recurrence -- is one lane per env, so a wave's access to a [K][n] array is 256 contiguous bytes.

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdlib>
#include <cstring>

#include "qg_host.h"

#define QGR_BLOCK 256
#define QGR_GAE_BLOCK 64          // one wave per workgroup: the recurrence is latency-bound, so the waves are spread over the CUs
#define QGR_GAE_DEPTH 16          // time steps whose loads are in flight ahead of the dependent chain

typedef float qgr_f32x4 __attribute__((ext_vector_type(4)));

#define QGR_SHARDS 32             // ticket counters, each on a 128-byte line of its own

struct QgrCtl {
    int32_t pos;                      // the cursor: slots [0, pos) are filled
    uint32_t pad;
    unsigned long long overflow;      // adds refused because the buffer was full
    unsigned long long bad_index;     // gather indices outside [0, pos * n)
    // Tickets of the running begin / add launch, all 0 between launches.  Arrivals on ONE counter are served one after the other
    // (some 12 ns each: 9 us for the 736 workgroups of an add at 4096 envs), so workgroup b draws from shard b % QGR_SHARDS and
    // the last arrival of a shard draws from the master: two short queues instead of one long one.
    struct alignas(128) {
        uint32_t count;
    } master, shard[QGR_SHARDS];
};

// What begin and add do first, every thread of every workgroup: returns the cursor as the launch found it.  Lane 0 reads the cursor,
// hands it to the workgroup through LDS and then -- off the other waves' path -- draws its tickets: the workgroup with the last ticket
// of its shard draws from the master, the one with the master's last ticket calls `next(p)`, which stores the new cursor.
// Ordering without a fence: the value of lane 0's load has come back before it can be written to LDS, so before the barrier, and
// the ticket is issued after the barrier; a workgroup draws from the master only with its shard ticket's value in hand, and stores
// the cursor only with the master's.  So every workgroup's read has COMPLETED before the store is issued.  The tickets are relaxed
// agent-scope adds on purpose: an acquire or a release at agent scope writes back and invalidates the L2 of the issuing XCD, once
// per workgroup and in the middle of the copies -- measured, 17 us per add at 4096 envs against 5 -- and there is no payload to
// publish: what the next launch reads goes through the kernel boundary.
template <class Next>
__device__ __forceinline__ int32_t qgr_cursor(QgrCtl *ctl, Next next) {
    __shared__ int32_t sh_p;
    int32_t p = 0;
    if (threadIdx.x == 0) {
        p = __hip_atomic_load(&ctl->pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sh_p = p;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t G = gridDim.x, s = blockIdx.x % QGR_SHARDS;
        const uint32_t in_shard = (G - s + QGR_SHARDS - 1) / QGR_SHARDS, shards = G < QGR_SHARDS ? G : QGR_SHARDS;
        if (__hip_atomic_fetch_add(&ctl->shard[s].count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_shard - 1) {
            __hip_atomic_store(&ctl->shard[s].count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__hip_atomic_fetch_add(&ctl->master.count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == shards - 1) {
                __hip_atomic_store(&ctl->master.count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                next(p);
            }
        }
    }
    return sh_p;
}

// item `idx` of a copy of `rows` rows of D floats: W floats from src (row stride sstride) to dst (row stride dstride)
template <bool VEC>
__device__ __forceinline__ void qgr_copy_item(uint64_t idx, uint64_t rows, int D, const float *src, int64_t sstride, float *dst,
                                              int64_t dstride) {
    constexpr int W = VEC ? 4 : 1;
    const uint32_t per_row = (uint32_t)(D / W);
    const uint64_t total = rows * per_row;
    if (idx >= total) return;
    uint64_t row;
    uint32_t cv;
    if (total <= 0xffffffffull) {
        row = (uint32_t)idx / per_row;
        cv = (uint32_t)idx - (uint32_t)row * per_row;
    } else {
        row = idx / per_row;
        cv = (uint32_t)(idx - row * per_row);
    }
    const float *s = src + row * sstride + (size_t)cv * W;
    float *d = dst + row * dstride + (size_t)cv * W;
    if constexpr (VEC) *(qgr_f32x4 *)d = *(const qgr_f32x4 *)s;
    else *d = *s;
}

template <bool VEC>
__global__ __launch_bounds__(QGR_BLOCK) void qg_rollout_begin_kernel(int n, int D, QgrCtl *ctl, float *obs, const float *first,
                                                                    int first_stride) {
    const int32_t p = qgr_cursor(ctl, [&](int32_t) { __hip_atomic_store(&ctl->pos, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
    const uint64_t idx = (uint64_t)blockIdx.x * QGR_BLOCK + threadIdx.x;
    if (first) qgr_copy_item<VEC>(idx, (uint64_t)n, D, first, first_stride, obs, D);
    else if (p > 0) qgr_copy_item<VEC>(idx, (uint64_t)n, D, obs + (size_t)p * n * D, D, obs, D);
}

struct KRolloutAdd {
    int32_t n, K, D, A;
    int32_t obs_blocks, act_blocks;   // workgroups [0, obs_blocks) copy next_obs, the next act_blocks the actions, the rest the scalars
    int32_t next_obs_stride, reward_stride, done_kind, done_stride, episode_reward_stride;
    float gamma;
    // the caller's rows of this step
    const float *next_obs, *act, *log_prob, *value, *reward, *trunc_value, *episode_reward;
    const void *done;
    // the storage
    float *obs, *actions, *log_probs, *values, *rewards;
    uint8_t *dones;
    // the episode accumulators, one word per env each
    double *cur_return, *fin_return;
    long long *cur_length, *fin_length, *fin_count;
};

template <bool VEC>
__global__ __launch_bounds__(QGR_BLOCK) void qg_rollout_add_kernel(KRolloutAdd a, QgrCtl *ctl) {
    const int32_t K = a.K;
    const int32_t p = qgr_cursor(ctl, [&](int32_t q) {
        if (q < K) __hip_atomic_store(&ctl->pos, q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else atomicAdd(&ctl->overflow, 1ull);
    });
    if (p >= K || p < 0) return;                                       // full: nothing is stored (uniform over the grid)
    const size_t slot = (size_t)p * a.n;
    int b = blockIdx.x;
    if (b < a.obs_blocks) {
        qgr_copy_item<VEC>((uint64_t)b * QGR_BLOCK + threadIdx.x, (uint64_t)a.n, a.D, a.next_obs, a.next_obs_stride,
                           a.obs + (slot + a.n) * a.D, a.D);
        return;
    }
    b -= a.obs_blocks;
    if (b < a.act_blocks) {
        const uint64_t j = (uint64_t)b * QGR_BLOCK + threadIdx.x;
        if (j < (uint64_t)a.n * a.A) a.actions[slot * a.A + j] = a.act[j];
        return;
    }
    b -= a.act_blocks;
    const uint64_t i = (uint64_t)b * QGR_BLOCK + threadIdx.x;
    if (i >= (uint64_t)a.n) return;
    const float r = a.reward[i * a.reward_stride];
    const bool d = qg_done_at(a.done, a.done_kind, a.done_stride, i);
    a.log_probs[slot + i] = a.log_prob[i];
    a.values[slot + i] = a.value[i];
    a.dones[slot + i] = d ? 1 : 0;
    a.rewards[slot + i] = a.trunc_value ? fmaf(a.gamma, a.trunc_value[i], r) : r;      // one rounding: fused
    // the episode of env i (f64 return, integer length): this thread owns all five words
    const double ret = a.cur_return[i] + (double)(a.episode_reward ? a.episode_reward[i * a.episode_reward_stride] : r);
    const long long len = a.cur_length[i] + 1;
    if (d) {
        a.fin_return[i] += ret;
        a.fin_length[i] += len;
        a.fin_count[i] += 1;
        a.cur_return[i] = 0.0;
        a.cur_length[i] = 0;
    } else {
        a.cur_return[i] = ret;
        a.cur_length[i] = len;
    }
}

// The recurrence, in this rounding order (quadgym.h): with g = f32(gamma), gl = f32(gamma * gae_lambda) (the product formed in f64),
//   delta = fl(fma(g * nnt, nv, r) - v)      A = fma(gl * nnt, A', delta)      returns = fl(A + v)
// g * nnt and gl * nnt are exact (nnt is 0 or 1): four roundings per step.
__global__ __launch_bounds__(QGR_GAE_BLOCK) void qg_rollout_gae_kernel(int n, const QgrCtl *ctl, float g, float gl,
                                                                      const float *__restrict__ rewards,
                                                                      const float *__restrict__ values,
                                                                      const uint8_t *__restrict__ dones,
                                                                      const float *__restrict__ last_values,
                                                                      float *__restrict__ advantages, float *__restrict__ returns) {
#pragma clang fp contract(off)
    const int F = ctl->pos;
    const int i = blockIdx.x * QGR_GAE_BLOCK + threadIdx.x;
    if (i >= n || F < 1) return;
    constexpr int U = QGR_GAE_DEPTH;
    float nv = last_values[i], adv = 0.f;
    for (int t = F - 1; t >= 0; t -= U) {
        float r[U], v[U];
        uint8_t d[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t at = (size_t)max(t - u, 0) * n + i;
            r[u] = rewards[at], v[u] = values[at], d[u] = dones[at];
        }
#pragma unroll
        for (int u = 0; u < U; u++)
            if (t - u >= 0) {
                const size_t at = (size_t)(t - u) * n + i;
                const float gn = d[u] ? 0.f : g, gln = d[u] ? 0.f : gl;
                const float delta = fmaf(gn, nv, r[u]) - v[u];
                adv = fmaf(gln, adv, delta);
                advantages[at] = adv;
                returns[at] = adv + v[u];
                nv = v[u];
            }
    }
}

struct KRolloutGather {
    int32_t n, D, A, B;
    int32_t obs_blocks, act_blocks;   // as in KRolloutAdd; obs_blocks / act_blocks are 0 where that output is NULL
    const float *obs, *actions, *log_probs, *values, *advantages, *returns;
    float *o_obs, *o_actions, *o_log_prob, *o_values, *o_advantages, *o_returns;
};

template <bool VEC>
__global__ __launch_bounds__(QGR_BLOCK) void qg_rollout_gather_kernel(KRolloutGather a, QgrCtl *ctl, const int64_t *__restrict__ idx) {
    const int64_t valid = (int64_t)ctl->pos * a.n;
    int b = blockIdx.x;
    if (b < a.obs_blocks) {
        constexpr int W = VEC ? 4 : 1;
        const uint32_t per_row = (uint32_t)(a.D / W);
        const uint64_t item = (uint64_t)b * QGR_BLOCK + threadIdx.x;
        if (item >= (uint64_t)a.B * per_row) return;
        const uint32_t row = (uint32_t)(item / per_row), c = ((uint32_t)(item - (uint64_t)row * per_row)) * W;
        const int64_t f = idx[row];
        const bool ok = f >= 0 && f < valid;
        float *dst = a.o_obs + (size_t)row * a.D + c;
        if constexpr (VEC) {
            qgr_f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok) v = *(const qgr_f32x4 *)(a.obs + (size_t)f * a.D + c);
            *(qgr_f32x4 *)dst = v;
        } else {
            *dst = ok ? a.obs[(size_t)f * a.D + c] : 0.f;
        }
        return;
    }
    b -= a.obs_blocks;
    if (b < a.act_blocks) {
        const uint64_t item = (uint64_t)b * QGR_BLOCK + threadIdx.x;
        if (item >= (uint64_t)a.B * a.A) return;
        const uint32_t row = (uint32_t)(item / (uint32_t)a.A), c = (uint32_t)(item - (uint64_t)row * a.A);
        const int64_t f = idx[row];
        a.o_actions[item] = (f >= 0 && f < valid) ? a.actions[(size_t)f * a.A + c] : 0.f;
        return;
    }
    b -= a.act_blocks;
    const int64_t row = (int64_t)b * QGR_BLOCK + threadIdx.x;
    if (row >= a.B) return;
    const int64_t f = idx[row];
    const bool ok = f >= 0 && f < valid;
    if (!ok) atomicAdd(&ctl->bad_index, 1ull);
    if (a.o_log_prob) a.o_log_prob[row] = ok ? a.log_probs[f] : 0.f;
    if (a.o_values) a.o_values[row] = ok ? a.values[f] : 0.f;
    if (a.o_advantages) a.o_advantages[row] = ok ? a.advantages[f] : 0.f;
    if (a.o_returns) a.o_returns[row] = ok ? a.returns[f] : 0.f;
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
struct qg_rollout {
    int32_t device;
    qg_rollout_desc desc;
    qg_rollout_storage st;
    float g, gl;              // f32(gamma), f32(gamma * gae_lambda)
    QgDevMem mem;
    QgrCtl *d_ctl;
    double *d_cur_return, *d_fin_return;         // [n_envs] each
    long long *d_cur_length, *d_fin_length, *d_fin_count;
};

static int rollout_validate(const qg_rollout_desc *d, const qg_rollout_storage *s) {
    if (!d) return fail(QG_ERR_ARG, "qg_rollout: null description");
    QG_CHECK_STRUCT(d, qg_rollout_desc);
    if (d->n_envs < 1) return fail(QG_ERR_ARG, "qg_rollout: n_envs %d must be >= 1", d->n_envs);
    if (d->n_steps < 1) return fail(QG_ERR_ARG, "qg_rollout: n_steps %d must be >= 1", d->n_steps);
    if (d->obs_dim < 1 || d->obs_dim > 512) return fail(QG_ERR_ARG, "qg_rollout: obs_dim %d outside 1 .. 512", d->obs_dim);
    if (d->act_dim < 1 || d->act_dim > 16) return fail(QG_ERR_ARG, "qg_rollout: act_dim %d outside 1 .. 16", d->act_dim);
    if (!qg_finite64(d->gamma) || d->gamma < 0.0 || d->gamma > 1.0)
        return fail(QG_ERR_ARG, "qg_rollout: gamma %g must be finite and in [0, 1]", d->gamma);
    if (!qg_finite64(d->gae_lambda) || d->gae_lambda < 0.0 || d->gae_lambda > 1.0)
        return fail(QG_ERR_ARG, "qg_rollout: gae_lambda %g must be finite and in [0, 1]", d->gae_lambda);
    if (((int64_t)d->n_steps + 1) * d->n_envs > INT32_MAX)
        return fail(QG_ERR_ARG, "qg_rollout: (n_steps + 1) * n_envs = %lld rows are more than 2^31 - 1",
                    (long long)(((int64_t)d->n_steps + 1) * d->n_envs));
    if (!s) return fail(QG_ERR_ARG, "qg_rollout: null storage");
    QG_CHECK_STRUCT(s, qg_rollout_storage);
    const void *f32s[] = {s->obs, s->actions, s->log_prob, s->values, s->rewards, s->advantages, s->returns};
    const char *names[] = {"obs", "actions", "log_prob", "values", "rewards", "advantages", "returns"};
    for (int k = 0; k < 7; k++) {
        if (!f32s[k]) return fail(QG_ERR_ARG, "qg_rollout_storage.%s is NULL", names[k]);
        if (!qg_aligned(f32s[k], sizeof(float))) return fail(QG_ERR_ARG, "qg_rollout_storage.%s is not aligned to 4 bytes", names[k]);
    }
    if (!s->dones) return fail(QG_ERR_ARG, "qg_rollout_storage.dones is NULL");
    return QG_OK;
}

extern "C" int qg_rollout_destroy(qg_rollout *p) {
    if (p) qg_free_handle(p, p->device);           // launches may still be in flight on a caller's stream
    return QG_OK;
}

extern "C" int qg_rollout_create(int32_t device_id, const qg_rollout_desc *desc, const qg_rollout_storage *storage, qg_rollout **out) {
    if (!out) return fail(QG_ERR_ARG, "qg_rollout_create: null output");
    *out = nullptr;
    QG_TRY(rollout_validate(desc, storage));
    QG_TRY(qg_open_device(device_id, nullptr));
    qg_rollout *p = qg_new_handle<qg_rollout>();
    if (!p) return QG_ERR_ALLOC;
    p->device = device_id;
    p->desc = *desc;
    p->st = *storage;
    p->g = (float)desc->gamma;
    p->gl = (float)(desc->gamma * desc->gae_lambda);
    const size_t n = (size_t)desc->n_envs;
    if (p->mem.alloc(p->d_ctl, sizeof(QgrCtl), true) || p->mem.alloc(p->d_cur_return, n * sizeof(double), true) ||
        p->mem.alloc(p->d_fin_return, n * sizeof(double), true) || p->mem.alloc(p->d_cur_length, n * sizeof(long long), true) ||
        p->mem.alloc(p->d_fin_length, n * sizeof(long long), true) || p->mem.alloc(p->d_fin_count, n * sizeof(long long), true)) {
        qg_rollout_destroy(p);
        return QG_ERR_ALLOC;
    }
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        qg_rollout_destroy(p);
        return fail(QG_ERR_DEVICE, "qg_rollout_create: %s", hipGetErrorString(e));
    }
    *out = p;
    return QG_OK;
}

// workgroups of a copy of n rows of D floats, W floats per thread; QG_ERR_ARG where one launch does not take them
static int rollout_blocks(int64_t rows, int per_row, int64_t *blocks) {
    *blocks = (rows * per_row + QGR_BLOCK - 1) / QGR_BLOCK;
    if (*blocks > INT32_MAX / 2) return fail(QG_ERR_ARG, "qg_rollout: %lld rows of %d items are more than one launch takes", (long long)rows, per_row);
    return QG_OK;
}

extern "C" int qg_rollout_begin_device(qg_rollout *p, const float *obs, int32_t obs_stride, void *stream) {
    if (!p) return fail(QG_ERR_ARG, "qg_rollout_begin_device: null handle");
    const int D = p->desc.obs_dim, n = p->desc.n_envs;
    if (obs && obs_stride < D) return fail(QG_ERR_ARG, "qg_rollout_begin_device: obs_stride %d < obs_dim %d", obs_stride, D);
    if (obs && !qg_aligned(obs, sizeof(float))) return fail(QG_ERR_ARG, "qg_rollout_begin_device: obs is not aligned to 4 bytes");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    const bool vec = D % 4 == 0 && qg_aligned(p->st.obs, 16) && (!obs || (obs_stride % 4 == 0 && qg_aligned(obs, 16)));
    int64_t blocks;
    QG_TRY(rollout_blocks(n, D / (vec ? 4 : 1), &blocks));
    const hipStream_t st = (hipStream_t)stream;
    if (vec) qg_rollout_begin_kernel<true><<<(unsigned)blocks, QGR_BLOCK, 0, st>>>(n, D, p->d_ctl, p->st.obs, obs, obs_stride);
    else qg_rollout_begin_kernel<false><<<(unsigned)blocks, QGR_BLOCK, 0, st>>>(n, D, p->d_ctl, p->st.obs, obs, obs_stride);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_rollout_add_device(qg_rollout *p, const qg_rollout_step *s, void *stream) {
    if (!s) return fail(QG_ERR_ARG, "qg_rollout_add_device: null step");
    QG_CHECK_STRUCT(s, qg_rollout_step);
    if (!p) return fail(QG_ERR_ARG, "qg_rollout_add_device: null handle");
    if (!s->next_obs || !s->actions || !s->log_prob || !s->value || !s->reward || !s->done)
        return fail(QG_ERR_ARG, "qg_rollout_add_device: next_obs, actions, log_prob, value, reward and done must not be NULL");
    const int D = p->desc.obs_dim, n = p->desc.n_envs, A = p->desc.act_dim;
    if (s->next_obs_stride < D) return fail(QG_ERR_ARG, "qg_rollout_add_device: next_obs_stride %d < obs_dim %d", s->next_obs_stride, D);
    // (both strides ahead of done_kind, as ever: qg_check_done alone would look at done_kind first)
    if (s->reward_stride < 1 || s->done_stride < 1)
        return fail(QG_ERR_ARG, "qg_rollout_add_device: reward_stride %d and done_stride %d must be >= 1", s->reward_stride, s->done_stride);
    QG_TRY(qg_check_done("qg_rollout_add_device", s->done, s->done_kind, s->done_stride));
    if (s->episode_reward && s->episode_reward_stride < 1)
        return fail(QG_ERR_ARG, "qg_rollout_add_device: episode_reward_stride must be >= 1");
    const void *f32s[] = {s->next_obs, s->actions, s->log_prob, s->value, s->reward, s->trunc_value, s->episode_reward,
                          s->done_kind == QG_DONE_F32 ? s->done : nullptr};
    for (const void *q : f32s)
        if (!qg_aligned(q, sizeof(float))) return fail(QG_ERR_ARG, "qg_rollout_add_device: a float pointer is not aligned to 4 bytes");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    KRolloutAdd a;
    memset(&a, 0, sizeof a);
    a.n = n, a.K = p->desc.n_steps, a.D = D, a.A = A;
    a.next_obs_stride = s->next_obs_stride, a.reward_stride = s->reward_stride;
    a.done_kind = s->done_kind, a.done_stride = s->done_stride, a.episode_reward_stride = s->episode_reward_stride;
    a.gamma = p->g;
    a.next_obs = s->next_obs, a.act = s->actions, a.log_prob = s->log_prob, a.value = s->value, a.reward = s->reward;
    a.trunc_value = s->trunc_value, a.episode_reward = s->episode_reward, a.done = s->done;
    a.obs = p->st.obs, a.actions = p->st.actions, a.log_probs = p->st.log_prob, a.values = p->st.values, a.rewards = p->st.rewards;
    a.dones = p->st.dones;
    a.cur_return = p->d_cur_return, a.fin_return = p->d_fin_return;
    a.cur_length = p->d_cur_length, a.fin_length = p->d_fin_length, a.fin_count = p->d_fin_count;
    const bool vec = D % 4 == 0 && s->next_obs_stride % 4 == 0 && qg_aligned(s->next_obs, 16) && qg_aligned(p->st.obs, 16);
    int64_t ob, ab;
    QG_TRY(rollout_blocks(n, D / (vec ? 4 : 1), &ob));
    QG_TRY(rollout_blocks(n, A, &ab));
    a.obs_blocks = (int32_t)ob, a.act_blocks = (int32_t)ab;
    const int64_t blocks = ob + ab + ((int64_t)n + QGR_BLOCK - 1) / QGR_BLOCK;
    if (blocks > INT32_MAX) return fail(QG_ERR_ARG, "qg_rollout_add_device: %d envs are more than one launch takes", n);
    const hipStream_t st = (hipStream_t)stream;
    if (vec) qg_rollout_add_kernel<true><<<(unsigned)blocks, QGR_BLOCK, 0, st>>>(a, p->d_ctl);
    else qg_rollout_add_kernel<false><<<(unsigned)blocks, QGR_BLOCK, 0, st>>>(a, p->d_ctl);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_rollout_compute_device(qg_rollout *p, const float *last_values, void *stream) {
    if (!p || !last_values) return fail(QG_ERR_ARG, "qg_rollout_compute_device: null argument");
    if (!qg_aligned(last_values, sizeof(float))) return fail(QG_ERR_ARG, "qg_rollout_compute_device: last_values is not aligned to 4 bytes");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    const int n = p->desc.n_envs;
    qg_rollout_gae_kernel<<<(unsigned)((n + QGR_GAE_BLOCK - 1) / QGR_GAE_BLOCK), QGR_GAE_BLOCK, 0, (hipStream_t)stream>>>(
        n, p->d_ctl, p->g, p->gl, p->st.rewards, p->st.values, p->st.dones, last_values, p->st.advantages, p->st.returns);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_rollout_gather_device(qg_rollout *p, const int64_t *idx, int32_t B, const qg_rollout_batch *out, void *stream) {
    if (!out) return fail(QG_ERR_ARG, "qg_rollout_gather_device: null batch");
    QG_CHECK_STRUCT(out, qg_rollout_batch);
    if (B < 1) return fail(QG_ERR_ARG, "qg_rollout_gather_device: B is %d, a batch has at least one row", B);
    if (!p || !idx) return fail(QG_ERR_ARG, "qg_rollout_gather_device: null argument");
    if (!qg_aligned(idx, sizeof(int64_t))) return fail(QG_ERR_ARG, "qg_rollout_gather_device: idx is not aligned to 8 bytes");
    const void *f32s[] = {out->obs, out->actions, out->old_log_prob, out->old_values, out->advantages, out->returns};
    for (const void *q : f32s)
        if (!qg_aligned(q, sizeof(float))) return fail(QG_ERR_ARG, "qg_rollout_gather_device: an output is not aligned to 4 bytes");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    const int D = p->desc.obs_dim, A = p->desc.act_dim;
    KRolloutGather a;
    memset(&a, 0, sizeof a);
    a.n = p->desc.n_envs, a.D = D, a.A = A, a.B = B;
    a.obs = p->st.obs, a.actions = p->st.actions, a.log_probs = p->st.log_prob, a.values = p->st.values;
    a.advantages = p->st.advantages, a.returns = p->st.returns;
    a.o_obs = out->obs, a.o_actions = out->actions, a.o_log_prob = out->old_log_prob, a.o_values = out->old_values;
    a.o_advantages = out->advantages, a.o_returns = out->returns;
    const bool vec = D % 4 == 0 && qg_aligned(p->st.obs, 16) && qg_aligned(out->obs, 16);
    int64_t ob = 0, ab = 0;
    if (out->obs) QG_TRY(rollout_blocks(B, D / (vec ? 4 : 1), &ob));
    if (out->actions) QG_TRY(rollout_blocks(B, A, &ab));
    a.obs_blocks = (int32_t)ob, a.act_blocks = (int32_t)ab;
    const int64_t blocks = ob + ab + ((int64_t)B + QGR_BLOCK - 1) / QGR_BLOCK;
    if (blocks > INT32_MAX) return fail(QG_ERR_ARG, "qg_rollout_gather_device: %d rows are more than one launch takes", B);
    const hipStream_t st = (hipStream_t)stream;
    if (vec) qg_rollout_gather_kernel<true><<<(unsigned)blocks, QGR_BLOCK, 0, st>>>(a, p->d_ctl, idx);
    else qg_rollout_gather_kernel<false><<<(unsigned)blocks, QGR_BLOCK, 0, st>>>(a, p->d_ctl, idx);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_rollout_get_info(qg_rollout *p, qg_rollout_info *info) {
    if (!p || !info) return fail(QG_ERR_ARG, "qg_rollout_get_info: null argument");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);         // an add may be in flight on a caller's stream
    QgrCtl h;
    HIP_TRY(hipMemcpy(&h, p->d_ctl, sizeof h, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    info->pos = h.pos;
    info->reserved = 0;
    info->overflow = (int64_t)h.overflow;
    info->bad_index = (int64_t)h.bad_index;
    return QG_OK;
}

extern "C" int qg_rollout_episode_stats(qg_rollout *p, double *return_sum, int64_t *length_sum, int64_t *count, int32_t clear) {
    if (!p || !return_sum || !length_sum || !count) return fail(QG_ERR_ARG, "qg_rollout_episode_stats: null argument");
    HIP_TRY(hipSetDevice(p->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    const size_t n = (size_t)p->desc.n_envs;
    QgHostBuf<double> hr(n);
    QgHostBuf<long long> hl(2 * n);
    QG_TRY(hr.oom());
    QG_TRY(hl.oom());
    HIP_TRY(hipMemcpy(hr, p->d_fin_return, n * sizeof(double), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(hl, p->d_fin_length, n * sizeof(long long), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(hl + n, p->d_fin_count, n * sizeof(long long), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    if (clear) {
        HIP_TRY(hipMemset(p->d_fin_return, 0, n * sizeof(double)), QG_ERR_DEVICE);
        HIP_TRY(hipMemset(p->d_fin_length, 0, n * sizeof(long long)), QG_ERR_DEVICE);
        HIP_TRY(hipMemset(p->d_fin_count, 0, n * sizeof(long long)), QG_ERR_DEVICE);
        HIP_TRY(hipDeviceSynchronize(), QG_ERR_DEVICE);
    }
    double rs = 0.0;
    int64_t ls = 0, cs = 0;
    for (size_t i = 0; i < n; i++) rs += hr[i], ls += hl[i], cs += hl[n + i];          // in env order
    *return_sum = rs, *length_sum = ls, *count = cs;
    return QG_OK;
}
