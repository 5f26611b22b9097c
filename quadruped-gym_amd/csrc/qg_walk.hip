// qg_walk.hip -- the walking task layer, kernels and host side (qg_walk_*): what
// WalkingQuadrupedEnv adds around QuadrupedEnv.step() in antopio26/quadruped-gym
// (src/envs/walking_quad.py:96-148 step/reset bookkeeping, :162-428 the reward stack,
// src/envs/math_utils.py:11-158 the online frequency/amplitude estimator of the control signal,
// src/envs/control_inputs.py the velocity/heading command).
//
// Per env-step, in the reference's order (walking_quad.py:128-148):
//   qg_walk_pre_kernel   one thread per (channel, env): the estimator takes data.ctrl (the PREVIOUS applied
//                        action, :136), every thread writes its entry of the effective action (joint centres
//                        while data.time < settling_time, :142-143);
//   qg_step_kernel*      the physics, with flip + time-limit terminations (:156-166);
//   qg_walk_post_kernel  one thread per env: the ideal position integrates the commanded global velocity (:93,133; nothing
//                        between reads it), the 11 reward terms of input_control_reward (:352-428) on the step's
//                        sensordata and data.ctrl, their sum, episode bookkeeping of envs that finished.
// These three launches serve the one-env-per-lane and two-legs-per-lane mappings; with the default one-leg-per-lane mapping the
// whole walking env-step is ONE launch: qg_step_kernel_quad<.., WALK = true> (qg_kernel_quad.hip) runs the estimator update of
// its three channels per lane in the prologue and the reward in the epilogue, through the same device functions
// (qg_walk_dev.h).
// The estimator's amplitude is max - min over a sliding window of 2 / (min_freq * dt) samples (250 at frame_skip
// 4).  Scanning the window every step streams 12 KB per env (measured 62.7 us per launch at 4096 envs, 3x the
// physics), so the ring buffer carries per-block (16 samples) max / min summaries: a step re-reduces the one block
// that received the new sample and combines it with the other blocks' summaries -- 16 + 2*15 values instead of
// 250, bit-identical results (max / min are exact).  Buffers are laid out [slot][channel][env] so that consecutive
// threads touch consecutive addresses.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>
#include <cmath>
#include <cstring>

#include "qg_sim.h"          // qg_sim, qg_walk; through it qg_walk_dev.h: KWalkParams / KWalkState and the per-env device functions
                             // (shared with the fused step kernels)
#include "qg_tables.h"

// one thread per (env, channel): thread t = env * 12 + channel
__global__ void qg_walk_pre_kernel(KWalkParams P, KWalkState S, int n, const float *__restrict__ actions, const float *__restrict__ data_ctrl,
                                   const int32_t *__restrict__ nstep) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 12 * n) return;
    const int env = t / 12, ch = t - env * 12;
    // effective action: the joint centres while the robot settles (walking_quad.py:142-143)
    const bool settle = nstep[env] < P.settle_substeps;
    S.eff_actions[(size_t)env * 12 + ch] = settle ? P.joint_centers[ch] : actions[(size_t)env * 12 + ch];
    const int tt[1] = {t};
    const float xx[1] = {data_ctrl[ch * n + env]};     // data.ctrl is physics state: [12][n]
    const int calls = S.calls[env];
    WalkEstIn<1> in;
    float f_new[1], a_new[1];
    walk_estimator_load_n<1>(P, S, n, tt, calls, in);                     // math_utils.py:53-131 with data.ctrl (:136)
    walk_estimator_finish_n<1>(P, S, n, tt, xx, calls, in, f_new, a_new);
}

// one thread per env.  `sample_here`: redraw the command of the envs the step has auto-reset (random_controls on the device);
// off when a partially observable pack follows, which still has to show the old command and redraws afterwards itself.
__global__ void qg_walk_post_kernel(KWalkParams P, KWalkState S, int n, const float *__restrict__ obs /* [n][33] */,
                                    const uint8_t *__restrict__ done, float *__restrict__ reward, float *__restrict__ comps /* [n][11] or NULL */,
                                    int sample_here, uint64_t seed, uint64_t env_index_base, const int32_t *__restrict__ episode) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= n) return;
    WalkSums sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        float c = S.eff_actions[(size_t)env * 12 + j];               // data.ctrl after the step
        c = fminf(fmaxf(c, -1.f), 1.f);                              // quadruped.py:160
        walk_channel_terms(S, env, j, walk_channel_targets(P, j), c, S.prev_ctrl[env * 12 + j], S.f_est[env * 12 + j], S.a_est[env * 12 + j], sum);
        S.prev_ctrl[env * 12 + j] = c;
    }
    // the physics reset has already advanced the env's episode counter: the key of the episode that begins is episode - 1
    WalkEnvIn in = walk_env_load(S, n, env);
    in.episode_key = episode[env] - 1;
    walk_reward_env(P, S, n, env, obs + (size_t)env * 33, sum, in, done[env] != 0, reward, comps, sample_here, seed, env_index_base);
}

// the same draw for the envs `select` marks (NULL = all), as its own launch: explicit resets
__global__ void qg_walk_command_kernel(KWalkParams P, KWalkState S, int n, const uint8_t *__restrict__ select, uint64_t seed,
                                       uint64_t env_index_base, const int32_t *__restrict__ episode) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= n) return;
    if (select && !select[env]) return;
    walk_sample_command(P, S, n, env, seed, env_index_base, episode[env] - 1);
}

// explicit (masked) episode reset of the walking state
__global__ void qg_walk_reset_kernel(KWalkParams P, KWalkState S, int n, const uint8_t *mask) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= n) return;
    if (mask && !mask[env]) return;
    S.ideal[env] = 0.f; S.ideal[n + env] = 0.f;
    for (int j = 0; j < 12; ++j) S.prev_ctrl[env * 12 + j] = P.joint_centers[j];
    S.has_derive[env] = 0;
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
// The walking env-step is ONE launch with every mapping AUTO can pick -- the task layer is fused into the one-link-per-lane, the
// one-leg-per-lane and the two-legs-per-lane kernels (16.9 us at 4096 envs, 33.9 us at 32 768; estimator -> physics -> reward as
// three launches measured 33.0 and 46.7 us).  Only an explicit LANE request keeps the three launches.
bool qg_walk_fused(const qg_sim *s) { const int m = qg_effective_mapping(s); return m == QG_MAP_QUAD || m == QG_MAP_LINK || m == QG_MAP_PAIR; }

extern "C" int qg_walk_default_params(qg_walk_params *p) {
    if (!p) return fail(QG_ERR_ARG, "qg_walk_default_params: null output");
    memset(p, 0, sizeof *p);
    p->settling_time = 0.0;
    for (int i = 0; i < QG_NU; i++) {
        p->joint_centers[i] = (i % 3 == 2) ? -0.5 : 0.0;
        p->amp_target[i] = (i % 3 == 0) ? 1.5 : ((i % 3 == 1) ? 0.5 : 0.0);
        p->freq_target[i] = (i % 3 == 2) ? 0.0 : 1.0;
    }
    p->ema_alpha = 0.8;
    p->min_freq = 1.0;
    p->control_cost_alpha = 0.8;
    const double w[10] = {10.0, -2.0, 10.0, -50.0, 10.0, 10.0, -50.0, -1.0, -2.5, -8.0};
    for (int i = 0; i < 10; i++) p->w[i] = w[i];
    p->w_diff_ideal = -20.0;
    p->body_height = 0.13;
    return QG_OK;
}

extern "C" int qg_walk_destroy(qg_walk *w) {
    if (!w) return QG_OK;
    if (w->cmdcur) return fail(QG_ERR_ARG, "qg_walk_destroy: a command curriculum is bound to this layer (qg_cmdcur_destroy first)");
    (void)hipSetDevice(w->sim->device);
    (void)hipDeviceSynchronize();                  // steps that read the task state may still be in flight on a caller's stream
    if (w->bound) {                                // give the sim back as qg_walk_create found it
        qg_sim *s = w->sim;
        s->task.use_flip = w->saved_use_flip;
        s->track_ctrl = w->saved_track_ctrl;
        s->walk_bound -= 1;
        KModel km;
        KTask kt;
        if (build_tables(&s->model, &s->task, &km, &kt) == QG_OK) (void)hipMemcpy(s->d_task, &kt, sizeof kt, hipMemcpyHostToDevice);
    }
    w->mem.free_all();
    delete w;
    return QG_OK;
}

extern "C" int qg_walk_create(qg_sim *s, const qg_walk_params *params, qg_walk **out) {
    if (!s || !out) return fail(QG_ERR_ARG, "qg_walk_create: null argument");
    *out = nullptr;
    if (s->obs_dim != QG_NSENSOR) return fail(QG_ERR_ARG, "qg_walk_create: the walking rewards read the 33-value sensordata (obs_mode QG_OBS_FULL)");
    // one task layer per simulator: a second one would save the flags the first has already switched (flip termination, data.ctrl
    // tracking) as "what the sim had", and whichever is destroyed first would switch them off under the other
    if (s->walk_bound) return fail(QG_ERR_ARG, "qg_walk_create: a walking task layer is already bound to this simulator (destroy it first)");
    if (s->res.active) return fail(QG_ERR_ARG, "qg_walk_create: the resident step mode is on (qg_resident_stop first)");
    qg_walk_params dp;
    if (!params) { qg_walk_default_params(&dp); params = &dp; }
    if (!(params->min_freq > 0) || !(params->ema_alpha >= 0 && params->ema_alpha <= 1)) return fail(QG_ERR_ARG, "qg_walk_create: bad estimator parameters");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    qg_walk *w = qg_new_handle<qg_walk>();
    if (!w) return QG_ERR_ALLOC;
    w->sim = s;
    w->params = *params;
    const double dt = s->model.timestep * s->task.frame_skip;        // walking_quad.py:56,93
    KWalkParams &k = w->kp;
    k.dt = (float)dt;
    k.inv_dt = (float)(1.0 / dt);
    int64_t settle = params->settling_time > 0 ? qg_time_limit_substeps_impl(s->model.timestep, params->settling_time) : 0;
    k.settle_substeps = (int32_t)(settle > INT32_MAX ? INT32_MAX : settle);
    {   // the reference puts no upper bound on the window (frame_skip 1 / 2 / 3 at the shipped timestep: 1000 / 500 / 334 samples);
        // only memory does: the ring holds window x 12 x n_envs samples.  (Checked as a double BEFORE the conversion: a tiny min_freq
        // would make the cast itself undefined.)
        const double w_exact = std::ceil(2.0 / (params->min_freq * dt));   // math_utils.py:26-28
        if (!(w_exact >= 1) || w_exact > 1e6) {
            delete w;
            return fail(QG_ERR_ARG, "qg_walk_create: estimator window %g outside 1..1000000 samples (min_freq * timestep * frame_skip)", w_exact);
        }
        k.window = (int32_t)w_exact;
    }
    k.ema_alpha = (float)params->ema_alpha;
    k.control_cost_alpha = (float)params->control_cost_alpha;
    for (int i = 0; i < 10; i++) k.w[i] = (float)params->w[i];
    k.w_diff_ideal = (float)params->w_diff_ideal;
    k.body_height = (float)params->body_height;
    for (int i = 0; i < QG_NU; i++) {
        k.joint_centers[i] = (float)params->joint_centers[i];
        k.amp_target[i] = (float)params->amp_target[i];
        k.freq_target[i] = (float)params->freq_target[i];
    }
    k.auto_reset = s->task.auto_reset;
    k.unit_zero = params->unit_zero ? 1 : 0;
    const size_t n = (size_t)s->n, W = (size_t)k.window;
    // the ring in whole blocks and all 16 summary slots, whatever the window: the estimator's loads are unconditional
    const size_t nb = (W + QG_WALK_BLOCK - 1) / QG_WALK_BLOCK, Wp = nb * QG_WALK_BLOCK;
    const size_t nbs = nb > QG_WALK_MAXBLOCKS ? nb : QG_WALK_MAXBLOCKS;     // at least the 16 slots the unrolled rebuild reads
    const size_t sblock = (size_t)(QG_WALK_BLOCK + 1) * 12 * n * 4;
    w->ring_slots = Wp; w->summary_blocks = nbs;
    QgDevMem &M = w->mem;
    KWalkState &S = w->st;
    const bool Z = true;              // every array starts as zeros
    if (M.alloc(S.vel, 2 * n * 4, Z) || M.alloc(S.head, 2 * n * 4, Z) || M.alloc(S.gvel, 2 * n * 4, Z) || M.alloc(S.ideal, 2 * n * 4, Z) ||
        M.alloc(S.prev_ctrl, 12 * n * 4, Z) || M.alloc(S.prev_ctrl_cost, n * 4, Z) || M.alloc(S.has_ctrl_cost, n, Z) ||
        M.alloc(S.prev_derive, n * 4, Z) || M.alloc(S.has_derive, n, Z) || M.alloc(S.calls, n * 4, Z) ||
        M.alloc(S.sig, Wp * 12 * n * 4, Z) || M.alloc(S.cross, Wp * 12 * n, Z) || M.alloc(S.bmax, nbs * 12 * n * 4, Z) ||
        M.alloc(S.bmin, nbs * 12 * n * 4, Z) || M.alloc(S.smax, sblock, Z) || M.alloc(S.smin, sblock, Z) || M.alloc(S.count, 12 * n * 4, Z) ||
        M.alloc(S.f_est, 12 * n * 4, Z) || M.alloc(S.a_est, 12 * n * 4, Z) || M.alloc(S.eff_actions, 12 * n * 4, Z) ||
        M.alloc(w->d_obs, n * QG_NSENSOR * 4, Z) || M.alloc(w->d_reward, n * 4, Z) || M.alloc(w->d_comps, n * QG_NWALKREWARD * 4, Z) ||
        M.alloc(w->d_actions, n * 12 * 4, Z) || M.alloc(w->d_tmp, n * 12 * 4, Z) || M.alloc(w->d_done, n, Z)) {
        qg_walk_destroy(w);
        return QG_ERR_ALLOC;
    }
    // the reference's termination set for this env: flip or time limit (walking_quad.py:162-166); data.ctrl feeds the estimator
    w->saved_use_flip = s->task.use_flip;
    w->saved_track_ctrl = s->track_ctrl;
    w->bound = 1;
    s->walk_bound += 1;
    s->task.use_flip = 1;
    {
        KModel km;
        KTask kt;
        int rc = build_tables(&s->model, &s->task, &km, &kt);
        if (rc != QG_OK) { qg_walk_destroy(w); return rc; }
        hipError_t e = hipMemcpy(s->d_task, &kt, sizeof kt, hipMemcpyHostToDevice);
        if (e != hipSuccess) { qg_walk_destroy(w); return fail(QG_ERR_DEVICE, "task update: %s", hipGetErrorString(e)); }
    }
    s->track_ctrl = 1;
    *out = w;
    s->creating = 1;                     // the constructor's own reset does not count as an episode
    int rc = qg_walk_reset(w, nullptr, s->seed, 0);
    s->creating = 0;
    if (rc != QG_OK) { qg_walk_destroy(w); *out = nullptr; }
    return rc;
}

extern "C" int qg_walk_set_commands(qg_walk *w, const float *velocity_xy, const float *heading_xy) {
    if (!w || !velocity_xy || !heading_xy) return fail(QG_ERR_ARG, "qg_walk_set_commands: null argument");
    qg_sim *s = w->sim;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    size_t n = (size_t)s->n;
    QgHostBuf<float> host(6 * n);
    QG_TRY(host.oom());
    float *vel = host, *head = host + 2 * n, *gv = host + 4 * n;
    for (size_t i = 0; i < n; i++) {
        float v0 = velocity_xy[2 * i], v1 = velocity_xy[2 * i + 1], h0 = heading_xy[2 * i], h1 = heading_xy[2 * i + 1];
        vel[i] = v0; vel[n + i] = v1; head[i] = h0; head[n + i] = h1;
        gv[i] = h0 * v0 - h1 * v1;                    // control_inputs.py:14-27
        gv[n + i] = h1 * v0 + h0 * v1;
    }
    HIP_TRY(hipMemcpy(w->st.vel, vel, 2 * n * 4, hipMemcpyHostToDevice), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(w->st.head, head, 2 * n * 4, hipMemcpyHostToDevice), QG_ERR_DEVICE);
    HIP_TRY(hipMemcpy(w->st.gvel, gv, 2 * n * 4, hipMemcpyHostToDevice), QG_ERR_DEVICE);
    return QG_OK;
}

// new commands for the envs `select` marks (device pointer, NULL = all); no-op without a sampler
static int walk_sample_commands(qg_walk *w, const uint8_t *select, hipStream_t st) {
    if (!w->kp.cmd_sample) return QG_OK;
    qg_sim *s = w->sim;
    int threads = 256, blocks = (s->n + threads - 1) / threads;
    hipLaunchKernelGGL(qg_walk_command_kernel, dim3(blocks), dim3(threads), 0, st, w->kp, w->st, s->n, select, s->seed, s->env_index_base,
                       (const int32_t *)s->st.episode);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QG_ERR_LAUNCH, "qg_walk_command_kernel launch: %s", hipGetErrorString(e));
    return QG_OK;
}

extern "C" int qg_walk_set_command_sampler(qg_walk *w, const qg_command_sampler *c) {
    if (!w) return fail(QG_ERR_ARG, "null handle");
    if (c && w->cmdcur)
        return fail(QG_ERR_ARG, "qg_walk_set_command_sampler: a command curriculum is bound to this layer and draws its commands (qg_cmdcur_destroy first)");
    KWalkParams &k = w->kp;
    HIP_TRY(hipSetDevice(w->sim->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);   // steps reading the old parameters may be in flight
    if (!c) { k.cmd_sample = 0; return QG_OK; }
    if (c->fixed & ~7u) return fail(QG_ERR_ARG, "qg_walk_set_command_sampler: unknown bits in `fixed`");
    if (!(c->fixed & QG_CMD_FIXED_SPEED) && !(std::fabs(c->min_speed) < 1e30 && std::fabs(c->max_speed) < 1e30))
        return fail(QG_ERR_ARG, "qg_walk_set_command_sampler: min_speed / max_speed must be finite");
    k.cmd_fixed = c->fixed;
    k.cmd_min_speed = (float)c->min_speed;
    k.cmd_max_speed = (float)c->max_speed;
    k.cmd_theta = (float)c->fixed_heading_angle;
    k.cmd_alpha = (float)c->fixed_velocity_angle;
    k.cmd_speed = (float)c->fixed_speed;
    k.cmd_sample = 1;
    return QG_OK;
}

extern "C" int qg_walk_get_commands(qg_walk *w, float *velocity_xy, float *heading_xy) {
    if (!w) return fail(QG_ERR_ARG, "null handle");
    qg_sim *s = w->sim;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    size_t n = (size_t)s->n;
    QgHostBuf<float> host(2 * n);
    QG_TRY(host.oom());
    float *dsts[2] = {velocity_xy, heading_xy};
    const float *srcs[2] = {w->st.vel, w->st.head};
    for (int a = 0; a < 2; a++) {
        if (!dsts[a]) continue;
        HIP_TRY(hipMemcpy(host, srcs[a], 2 * n * 4, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
        for (size_t i = 0; i < n; i++) { dsts[a][2 * i] = host[i]; dsts[a][2 * i + 1] = host[n + i]; }
    }
    return QG_OK;
}

extern "C" int qg_walk_reset(qg_walk *w, const uint8_t *mask, uint64_t seed, uint32_t flags) {
    if (!w) return fail(QG_ERR_ARG, "null handle");
    qg_sim *s = w->sim;
    if ((flags & QG_RESET_DYNAMICS) && !s->dyn_range_set) return fail(QG_ERR_ARG, "qg_walk_reset: QG_RESET_DYNAMICS without a range (qg_set_dynamics_range)");
    QG_TRY(qg_reset(s, mask, seed, flags));            // uploads the mask into s->d_mask
    int threads = 256, blocks = (s->n + threads - 1) / threads;
    hipLaunchKernelGGL(qg_walk_reset_kernel, dim3(blocks), dim3(threads), 0, s->stream, w->kp, w->st, s->n, mask ? s->d_mask : nullptr);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    // walking_quad.py:121-122 (not for the constructor's own reset)
    if (!s->creating) QG_TRY(walk_sample_commands(w, mask ? s->d_mask : nullptr, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream), QG_ERR_LAUNCH);
    return QG_OK;
}

// pre + physics + post.  The commands of auto-reset envs are redrawn by the caller AFTER everything that still reads the old
// ones (the partially observable pack) has been launched.
int qg_walk_step_core(qg_walk *w, const float *actions, float *obs, float *reward, uint8_t *done, float *components, void *stream,
                      bool po_follows, const KPoLaunch *po_fused) {
    qg_sim *s = w->sim;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    hipStream_t st = (hipStream_t)stream;
    if (qg_walk_fused(s)) {
        KWalkLaunch wl;
        wl.P = w->kp;
        wl.S = w->st;
        wl.comps = components;
        wl.sample = (w->kp.cmd_sample && !po_follows) ? 1 : 0;
        return qg_launch_step(s, actions, obs, reward, done, nullptr, nullptr, st, &wl, po_fused);
    }
    if (po_fused) return fail(QG_ERR_ARG, "walk_step_core: no fused walking launch for this handle");
    int threads = 256;
    int total = 12 * s->n;
    hipLaunchKernelGGL(qg_walk_pre_kernel, dim3((total + threads - 1) / threads), dim3(threads), 0, st, w->kp, w->st, s->n, actions,
                       (const float *)s->st.ctrl, (const int32_t *)s->st.nstep);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    QG_TRY(qg_launch_step(s, w->st.eff_actions, obs, reward, done, nullptr, nullptr, st));
    hipLaunchKernelGGL(qg_walk_post_kernel, dim3((s->n + threads - 1) / threads), dim3(threads), 0, st, w->kp, w->st, s->n, (const float *)obs,
                       (const uint8_t *)done, reward, components, (w->kp.cmd_sample && !po_follows) ? 1 : 0, s->seed, s->env_index_base,
                       (const int32_t *)s->st.episode);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_walk_step_device(qg_walk *w, const float *actions, float *obs, float *reward, uint8_t *done, float *components, void *stream) {
    if (!w || !actions || !obs || !reward || !done) return fail(QG_ERR_ARG, "qg_walk_step_device: null argument");
    return qg_walk_step_core(w, actions, obs, reward, done, components, stream, false);
}

extern "C" int qg_walk_step(qg_walk *w, const float *actions, float *obs, float *reward, uint8_t *done, float *components) {
    if (!w || !actions || !obs || !reward || !done) return fail(QG_ERR_ARG, "qg_walk_step: null argument");
    qg_sim *s = w->sim;
    const size_t n = (size_t)s->n;
    const HostOut out[4] = {{obs, w->d_obs, n * QG_NSENSOR * 4}, {reward, w->d_reward, n * 4}, {done, w->d_done, n},
                            {components, w->d_comps, n * QG_NWALKREWARD * 4}};
    return host_step(s, actions, w->d_actions, out, [&] {
        return qg_walk_step_device(w, w->d_actions, w->d_obs, w->d_reward, w->d_done, components ? w->d_comps : nullptr, s->stream);
    });
}

extern "C" int qg_walk_get_estimates(qg_walk *w, float *f_est, float *a_est, float *ideal_xy) {
    if (!w) return fail(QG_ERR_ARG, "null handle");
    qg_sim *s = w->sim;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    // the estimates live env-major ([n][12]) on the device, as the caller wants them; the ideal position is [2][n]
    if (f_est) HIP_TRY(hipMemcpy(f_est, w->st.f_est, (size_t)s->n * 12 * 4, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    if (a_est) HIP_TRY(hipMemcpy(a_est, w->st.a_est, (size_t)s->n * 12 * 4, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    if (ideal_xy) {
        QG_TRY(qg_transpose_out_launch(s, w->st.ideal, w->d_tmp, 2));
        HIP_TRY(hipMemcpyAsync(ideal_xy, w->d_tmp, (size_t)s->n * 2 * 4, hipMemcpyDeviceToHost, s->stream), QG_ERR_DEVICE);
        HIP_TRY(hipStreamSynchronize(s->stream), QG_ERR_LAUNCH);
    }
    return QG_OK;
}

// ---- task-layer snapshot / restore (qg_sim.h) ------------------------------------------------------------------------------------
struct QgBlobHeader { uint32_t magic, version; int32_t n, window; int64_t bytes; };
#define QG_BLOB_WALK 0x4b4c5751u   /* "QWLK" */
#define QG_BLOB_VERSION 5u

static int walk_fields(const qg_walk *w, QgField *f) {
    const size_t n = (size_t)w->sim->n, R = w->ring_slots, NB = w->summary_blocks;
    const KWalkState &S = w->st;
    const QgField all[] = {
        {S.vel, 2 * n * 4}, {S.head, 2 * n * 4}, {S.gvel, 2 * n * 4}, {S.ideal, 2 * n * 4}, {S.prev_ctrl, 12 * n * 4}, {S.prev_ctrl_cost, n * 4},
        {S.has_ctrl_cost, n}, {S.prev_derive, n * 4}, {S.has_derive, n}, {S.calls, n * 4}, {S.sig, R * 12 * n * 4}, {S.cross, R * 12 * n},
        {S.bmax, NB * 12 * n * 4}, {S.bmin, NB * 12 * n * 4}, {S.smax, (size_t)(QG_WALK_BLOCK + 1) * 12 * n * 4}, {S.smin, (size_t)(QG_WALK_BLOCK + 1) * 12 * n * 4},
        {S.count, 12 * n * 4}, {S.f_est, 12 * n * 4},
        {S.a_est, 12 * n * 4}, {S.eff_actions, 12 * n * 4}};
    const int k = (int)(sizeof all / sizeof all[0]);
    if (f) memcpy(f, all, sizeof all);
    return k;
}
int64_t qg_blob_bytes(const QgField *f, int k) {
    size_t b = sizeof(QgBlobHeader);
    for (int i = 0; i < k; i++) b += f[i].bytes;
    return (int64_t)b;
}
int qg_blob_out(qg_sim *s, uint32_t magic, int32_t window, const QgField *f, int k, void *blob) {
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);   // steps may be in flight on a caller's stream
    QgBlobHeader h = {magic, QG_BLOB_VERSION, s->n, window, qg_blob_bytes(f, k)};
    uint8_t *p = (uint8_t *)blob;
    memcpy(p, &h, sizeof h);
    p += sizeof h;
    for (int i = 0; i < k; i++) {
        HIP_TRY(hipMemcpy(p, f[i].ptr, f[i].bytes, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
        p += f[i].bytes;
    }
    return QG_OK;
}
int qg_blob_in(qg_sim *s, uint32_t magic, int32_t window, const QgField *f, int k, const void *blob, const char *who) {
    QgBlobHeader h;
    memcpy(&h, blob, sizeof h);
    if (h.magic != magic || h.version != QG_BLOB_VERSION) return fail(QG_ERR_ARG, "%s: not a snapshot of this layer / library version", who);
    if (h.n != s->n || h.window != window || h.bytes != qg_blob_bytes(f, k))
        return fail(QG_ERR_ARG, "%s: the snapshot was taken from %d envs with window %d (%lld bytes); this layer has %d envs, window %d (%lld bytes)", who,
                    h.n, h.window, (long long)h.bytes, s->n, window, (long long)qg_blob_bytes(f, k));
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    const uint8_t *p = (const uint8_t *)blob + sizeof h;
    for (int i = 0; i < k; i++) {
        HIP_TRY(hipMemcpy(f[i].ptr, p, f[i].bytes, hipMemcpyHostToDevice), QG_ERR_DEVICE);
        p += f[i].bytes;
    }
    return QG_OK;
}

extern "C" int64_t qg_walk_state_bytes(const qg_walk *w) {
    if (!w) return fail(QG_ERR_ARG, "null handle");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_bytes(f, walk_fields(w, f));
}
extern "C" int qg_walk_get_state(qg_walk *w, void *blob) {
    if (!w || !blob) return fail(QG_ERR_ARG, "qg_walk_get_state: null argument");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_out(w->sim, QG_BLOB_WALK, w->kp.window, f, walk_fields(w, f), blob);
}
extern "C" int qg_walk_set_state(qg_walk *w, const void *blob) {
    if (!w || !blob) return fail(QG_ERR_ARG, "qg_walk_set_state: null argument");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_in(w->sim, QG_BLOB_WALK, w->kp.window, f, walk_fields(w, f), blob, "qg_walk_set_state");
}
