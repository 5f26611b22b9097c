// qg_capi.hip -- the core of the C ABI declared in include/quadgym.h: the simulator handle.
//
// Owns the error record, the handle's life (create / destroy) and its per-env device state (struct-of-arrays in HBM), converts the
// double-precision model/task descriptions into the kernarg-sized single-precision tables the kernels read, resets, decides which
// mapping a step runs and enqueues it (qg_launch_step, the device-pointer steps), and holds the task / mapping / track_ctrl setters,
// the reset streams and the debug entry points.  The rest of the simulator's host side is three units without device code: the
// host-pointer path (qg_sim_host.hip), many env-steps per launch (qg_sim_multi.hip), per-env dynamics and wrenches
// (qg_sim_modes.hip).  The step kernels, their launchers and the leaves of each mapping are translation units of
// their own, one per family (qg_kernel_link.hip, qg_kernel_quad.hip, qg_kernel_pair.hip; their entry points: qg_step_launch.h);
// this one compiles only the five small kernels of reset and state transfer.  The handles bound to a simulator (qg_comm.hip,
// qg_walk.hip, qg_po.hip) reach it through qg_sim.h; qg_policy.hip and qg_norm.hip share qg_host.h only.
// There is no CPU code path: every compute entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/quadgym.h"
#include "../../include/qg_model_data.h"
#include "qg_step_dev.h"       // the shared device code: the reset kernels below draw and place the start pose as the step kernels do
#include "qg_step_launch.h"
#include "qg_tables.h"

static thread_local char g_err[512] = "";

int qg_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char *qg_version(void) { return "quadgym 0.1.0 (gfx950)"; }
extern "C" const char *qg_last_error(void) { return g_err; }

// The step time is a staircase in the batch size (profiles/r03/map_sweep.txt, microseconds per env-step on an MI355X): flat at 11.8 up to
// 4096 envs (one wave of the one-link-per-lane kernel per SIMD), 18.3-19.0 for 4097 .. 16 384 (one wave of the one-leg-per-lane kernel
// per SIMD), 24.5-25.3 for 16 385 .. 32 768 (one wave of the two-legs-per-lane kernel per SIMD), then ~23 us per further 32 768 envs.
// The top of a stair costs no more per step than its foot: this returns the top of the stair `n_envs` stands on.
extern "C" int32_t qg_recommended_batch(int32_t n_envs, int32_t device_id) {
    const int simds = qg_device_simds(device_id);
    if (n_envs < 1) n_envs = 1;
    const int64_t link = (int64_t)simds * QGK_LINK_ENVS, quad = (int64_t)simds * QGK_QUAD_ENVS, pair = (int64_t)simds * QGK_PAIR_ENVS;
    int64_t r = n_envs <= link ? link : (n_envs <= quad ? quad : ((n_envs + pair - 1) / pair) * pair);
    return (int32_t)(r > INT32_MAX ? INT32_MAX : r);
}

extern "C" int qg_device_pci_bus_id(int32_t device_id, char *out, int32_t len) {
    if (!out || len < 16) return qg_fail(QG_ERR_ARG, "qg_device_pci_bus_id: need a buffer of at least 16 bytes");
    hipError_t e = hipDeviceGetPCIBusId(out, len, device_id);
    if (e != hipSuccess) return qg_fail(QG_ERR_DEVICE, "hipDeviceGetPCIBusId(%d): %s", device_id, hipGetErrorString(e));
    return QG_OK;
}

extern "C" int qg_default_model(qg_model *out) {
    if (!out) return fail(QG_ERR_ARG, "qg_default_model: null output");
    static const qg_model def = QG_MODEL_DEFAULT_INIT;
    *out = def;
    return QG_OK;
}

extern "C" int qg_default_task(qg_task *out) {
    if (!out) return fail(QG_ERR_ARG, "qg_default_task: null output");
    memset(out, 0, sizeof *out);
    out->frame_skip = 4;          // quadruped.py:44
    out->max_time = 10.0;         // quadruped.py:43
    out->use_time_limit = 1;      // quadruped.py:52
    out->use_fall = 0;
    out->fall_height = 0.2;       // README.md:87
    out->w_forward = 1.0;         // README.md:65-72
    out->w_ctrl = -0.1;
    out->alive_bonus = 1.0;
    out->obs_mode = QG_OBS_FULL;
    out->sensor_lag = 1;
    out->auto_reset = 0;
    out->reset_flags = 0;
    for (int i = 0; i < QG_NU; i++) out->default_ctrl[i] = (i % 3 == 2) ? -0.5 : 0.0;   // quadruped.py:124
    out->reset_joint_jitter = 0.1;
    return QG_OK;
}

extern "C" int64_t qg_time_limit_substeps(double timestep, double max_time) { return qg_time_limit_substeps_impl(timestep, max_time); }

// the resident kernel hands the state back, then whatever is in flight on any stream -- a caller's included -- has run
int qg_retire_and_sync(qg_sim *s) {
    QG_TRY(qg_resident_retire(s));
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_destroy(qg_sim *s) {
    if (!s) return QG_OK;
    (void)hipSetDevice(s->device);
    (void)qg_resident_retire(s);
    (void)hipDeviceSynchronize();                  // steps may still be in flight on a caller's stream (the header's ordering contract)
    qg_resident_free(s);
    s->mem.free_all();
    if (s->h_pin) (void)hipHostFree(s->h_pin);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
    return QG_OK;
}

extern "C" int qg_create(int32_t n_envs, int32_t device_id, const qg_model *model, const qg_task *task, uint64_t env_index_base,
                         qg_sim **out) {
    if (!out) return fail(QG_ERR_ARG, "qg_create: null output");
    *out = nullptr;
    if (n_envs < 1) return fail(QG_ERR_ARG, "qg_create: n_envs must be >= 1");
    qg_model dm;
    qg_task dt;
    if (!model) { qg_default_model(&dm); model = &dm; }
    if (!task) { qg_default_task(&dt); task = &dt; }
    KModel km;
    KTask kt;
    QG_TRY(build_tables(model, task, &km, &kt));
    int simds;
    QG_TRY(qg_open_device(device_id, &simds));

    qg_sim *s = new (std::nothrow) qg_sim();
    if (!s) return fail(QG_ERR_ALLOC, "out of host memory");
    memset(s, 0, sizeof *s);
    s->n = n_envs;
    s->device = device_id;
    s->obs_dim = task->obs_mode == QG_OBS_IMU ? 21 : QG_NSENSOR;
    s->model = *model;
    s->task = *task;
    s->env_index_base = env_index_base;
    s->track_ctrl = 1;
    { const char *e = getenv("QG_LINK_HELPERS"); s->link_helpers = e ? (atoi(e) != 0) : 1; }
    s->mapping = QG_MAP_AUTO;
    s->simds = simds;
    if (const char *e = getenv("QG_PO_UNFUSED")) s->po_unfused = atoi(e) != 0;
    {
        static const KModel baked = {QG_BAKED_FLOATS};
        s->model_baked = QG_BAKED_LEGS_IDENTICAL && memcmp(&km, &baked, sizeof km) == 0;
    }
    const size_t n = (size_t)n_envs;
    QgDevMem &M = s->mem;
    if (M.alloc(s->d_model, sizeof(KModel)) || M.alloc(s->d_task, sizeof(KTask)) || M.alloc(s->st.qpos, n * QG_NQ * sizeof(float)) ||
        M.alloc(s->st.qvel, n * QG_NV * sizeof(float)) || M.alloc(s->st.act, n * QG_NU * sizeof(float)) ||
        M.alloc(s->st.ctrl, n * QG_NU * sizeof(float)) || M.alloc(s->st.nstep, n * sizeof(int32_t)) ||
        M.alloc(s->st.episode, n * sizeof(int32_t)) || M.alloc(s->d_actions, n * QG_NU * sizeof(float)) ||
        M.alloc(s->d_obs, n * (QG_NSENSOR + 2) * sizeof(float)) || M.alloc(s->d_reward, n * sizeof(float)) ||
        M.alloc(s->d_comps, n * QG_NREWARD * sizeof(float)) ||
        M.alloc(s->d_stage, n * (QG_NQ + QG_NV + 2 * QG_NU) * sizeof(float)) ||     // all four state fields side by side (qg_get_state)
        M.alloc(s->d_done, n) || M.alloc(s->d_mask, n)) {
        qg_destroy(s);
        return QG_ERR_ALLOC;
    }
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&s->ev0);
    if (e == hipSuccess) e = hipEventCreate(&s->ev1);
    if (e == hipSuccess) e = hipMemcpy(s->d_model, &km, sizeof km, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_task, &kt, sizeof kt, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        qg_destroy(s);
        return fail(QG_ERR_DEVICE, "device setup: %s", hipGetErrorString(e));
    }
    if (hipMemset(s->st.episode, 0, n * sizeof(int32_t)) != hipSuccess) {
        qg_destroy(s);
        return fail(QG_ERR_DEVICE, "device setup: memset");
    }
    *out = s;
    s->creating = 1;                 // the constructor's own reset does not count as an episode
    const int rc = qg_reset(s, nullptr, 0, 0);
    s->creating = 0;
    if (rc != QG_OK) {
        qg_destroy(s);
        *out = nullptr;
    }
    return rc;
}

extern "C" int qg_num_envs(const qg_sim *s) { return s ? s->n : fail(QG_ERR_ARG, "null handle"); }
extern "C" int qg_obs_dim(const qg_sim *s) { return s ? s->obs_dim : fail(QG_ERR_ARG, "null handle"); }

// ------------------------------------------------------------------------------------------
// reset (quadruped.py:115-139): mj_resetData, time = 0, ctrl = default; optional random yaw and hinge jitter
// ------------------------------------------------------------------------------------------
__global__ void qg_reset_kernel(const KModel *__restrict__ M, const KTask *__restrict__ T, KState st, int n, const uint8_t *mask,
                                uint64_t seed, uint64_t env_index_base, uint32_t flags, int count_episode) {
    int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= n) return;
    if (mask && !mask[env]) return;
    const int ep = st.episode[env];
    for (int j = 0; j < 19; ++j) st.qpos[j * n + env] = M->qpos0[j];
    if (flags & 2u) {
        for (int j = 0; j < 12; ++j)
            st.qpos[(7 + j) * n + env] = jittered_hinge(M->qpos0[7 + j], M->link[j].lo, M->link[j].hi, T->reset_joint_jitter, seed,
                                                        env_index_base + (uint64_t)env, ep, j);
    }
    if (flags & 1u)
        QG_RESET_HEADING(seed, env_index_base + (uint64_t)env, ep, st.qpos[3 * n + env], st.qpos[4 * n + env], st.qpos[5 * n + env], st.qpos[6 * n + env]);
    for (int j = 0; j < 18; ++j) st.qvel[j * n + env] = 0.f;
    for (int j = 0; j < 12; ++j) { st.act[j * n + env] = 0.f; st.ctrl[j * n + env] = T->default_ctrl[j]; }
    st.nstep[env] = 0;
    if (count_episode) st.episode[env] += 1;
}

// QG_RESET_JOINT_JITTER for the envs the step kernel has just auto-reset: their hinges stand at qpos0 and their episode counter
// has advanced, so the key of the episode that begins is episode - 1 (the one its reset yaw used).  A separate launch, issued
// only when the task asks for jitter: inside the step kernels even a never-taken branch of this size measured +0.9 % at 4096
// envs and +2 % at 32 768 (same-box A/B).  One thread per (hinge, env); `done` is the step's done output, either as bytes
// or as the last column of the packed rows.
__global__ void qg_jitter_kernel(const KModel *__restrict__ M, const KTask *__restrict__ T, KState st, int n, const uint8_t *__restrict__ done,
                                 const float *__restrict__ packed, int row, uint64_t seed, uint64_t env_index_base) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 12 * n) return;
    const int j = t / n, env = t - j * n;
    const bool was_reset = done ? (done[env] != 0) : (packed[(size_t)env * row + (row - 1)] > 0.5f);
    if (!was_reset) return;
    st.qpos[(7 + j) * n + env] = jittered_hinge(M->qpos0[7 + j], M->link[j].lo, M->link[j].hi, T->reset_joint_jitter, seed,
                                                env_index_base + (uint64_t)env, st.episode[env] - 1, j);
}

// QG_RESET_DYNAMICS: column c of env i drawn for episode e as lo + (hi - lo) u, u = uniform24s(seed, base + i, e, 16 + c) -- streams of
// their own, so the yaw (0), hinge (1..12) and command (13..15) draws are the same with the flag as without.  One thread per (column,
// env).  Behind qg_reset (`mask`: the envs reset, NULL: all; key = the episode counter before the reset advances it, key_offset 0) and,
// as qg_jitter_kernel and for its reason, as a launch of its own behind a step that auto-resets (`done` bytes or the packed rows' last
// column: the envs that finished; their counter has advanced, key_offset -1).
#define QG_STREAM_DYNAMICS 16u
__global__ void qg_dyn_draw_kernel(float *__restrict__ rows, KDynRange R, const int32_t *__restrict__ episode, int n, const uint8_t *__restrict__ mask,
                                   const uint8_t *__restrict__ done, const float *__restrict__ packed, int row, int key_offset, uint64_t seed,
                                   uint64_t env_index_base) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= QGK_NDYN * n) return;
    const int c = t / n, env = t - c * n;
    if (mask && !mask[env]) return;
    if (!mask && (done || packed)) {
        const bool was_reset = done ? (done[env] != 0) : (packed[(size_t)env * row + (row - 1)] > 0.5f);
        if (!was_reset) return;
    }
    const float u = uniform24s(seed, env_index_base + (uint64_t)env, (uint64_t)(episode[env] + key_offset), QG_STREAM_DYNAMICS + (uint32_t)c);
    rows[(size_t)c * n + env] = fmaf(R.hi[c] - R.lo[c], u, R.lo[c]);
}

// env-major [n][w] <-> field-major [w][n] (state snapshot / restore at the ABI)
__global__ void qg_transpose_in(const float *__restrict__ src, float *__restrict__ dst, int n, int w) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * w) return;
    int f = i / n, e = i - f * n;
    dst[i] = src[(size_t)e * w + f];
}
__global__ void qg_transpose_out(const float *__restrict__ src, float *__restrict__ dst, int n, int w) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * w) return;
    int e = i / w, f = i - e * w;
    dst[i] = src[(size_t)f * n + e];
}

extern "C" int qg_reset(qg_sim *s, const uint8_t *mask, uint64_t seed, uint32_t flags) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    // steps may be in flight on a caller's stream (qg_step_device*): the reset runs on the library's own non-blocking stream
    // and must not overlap them (a resident step kernel first stores the state it holds in registers and leaves)
    QG_TRY(qg_retire_and_sync(s));
    // the seed keys the reset streams of EVERY env (auto-resets included): only a whole-batch reset may change it, a masked
    // reset draws from the streams already in force
    if ((flags & QG_RESET_DYNAMICS) && !s->dyn_range_set) return fail(QG_ERR_ARG, "qg_reset: QG_RESET_DYNAMICS without a range (qg_set_dynamics_range)");
    if (!mask) s->seed = seed;
    else seed = s->seed;
    const uint8_t *dmask = nullptr;
    if (mask) {
        HIP_TRY(hipMemcpyAsync(s->d_mask, mask, (size_t)s->n, hipMemcpyHostToDevice, s->stream), QG_ERR_DEVICE);
        dmask = s->d_mask;
    }
    int threads = 256, blocks = (s->n + threads - 1) / threads;
    if (flags & QG_RESET_DYNAMICS) {                 // keyed by the episode that begins: the counter before the reset kernel advances it
        const int total = QG_NDYN * s->n;
        hipLaunchKernelGGL(qg_dyn_draw_kernel, dim3((total + threads - 1) / threads), dim3(threads), 0, s->stream, s->d_dyn, s->dyn_range,
                           (const int32_t *)s->st.episode, s->n, dmask, (const uint8_t *)nullptr, (const float *)nullptr, 0, 0, seed, s->env_index_base);
        HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    }
    hipLaunchKernelGGL(qg_reset_kernel, dim3(blocks), dim3(threads), 0, s->stream, s->d_model, s->d_task, s->st, s->n, dmask, seed,
                       s->env_index_base, flags, s->creating ? 0 : 1);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    HIP_TRY(hipStreamSynchronize(s->stream), QG_ERR_LAUNCH);
    return QG_OK;
}

// AUTO = the measured optimum per batch size (profiles/r03/map_sweep.txt: every mapping around the boundaries on one box, HIP events,
// microseconds per launch at frame_skip 4):
//   envs        link     quad     pair
//   4 096       12.0     18.1              one link per lane: 1024 waves, one per SIMD
//   5 120       19.2     18.3              a second link wave per SIMD costs more than the quad kernel's idle SIMDs
//   16 384               19.0     24.2     one quad wave per SIMD
//   20 000               28.2     24.5     the quad grid needs a second wave on some SIMDs, the pair grid (32 envs per wave) does not
//   32 768               29.0     25.3
//   40 000               40.4     46.7     second round of pair waves (one wave per SIMD by construction) against two resident quad waves
//   57 344               51.9     47.5     from 1.75 rounds of pair waves on, pair is ahead again
//   262 144             187.7    187.6
// The one-env-per-lane kernel (66 us at 4096 envs) only runs on request.  The compiled-in robot runs the variants with literal
// constants; any other numbers run the variants that stage the model tables in LDS (link up to 4096 envs, quad above; no pair form).
int qg_effective_mapping(const qg_sim *s) {
    if (s->mapping == QG_MAP_LANE || s->mapping == QG_MAP_QUAD) return s->mapping;
    if (s->mapping == QG_MAP_PAIR) return qg_sim_baked(s) ? QG_MAP_PAIR : QG_MAP_QUAD;
    // (the one-link-per-lane kernel addresses the state with 32-bit byte offsets from scalar bases: 19 n floats must stay below 4 GiB)
    if (s->mapping == QG_MAP_LINK) return (s->task.sensor_lag && s->n <= (1 << 24)) ? QG_MAP_LINK : QG_MAP_QUAD;
    // up to one wave of the one-link-per-lane kernel per SIMD (4096 envs on the 1024 SIMDs of an MI355X); the other boundaries are
    // the same measurement in units of "waves per SIMD" (pair: > 1 quad wave per SIMD up to 1 pair wave per SIMD, and from 1.75 on)
    const int simds = s->simds;
    if (s->task.sensor_lag && s->n <= simds * QGK_LINK_ENVS) return QG_MAP_LINK;
    if (qg_sim_baked(s) && s->n > simds * QGK_QUAD_ENVS && (s->n <= simds * QGK_PAIR_ENVS || s->n >= (simds + 3 * (simds / 4)) * QGK_PAIR_ENVS)) return QG_MAP_PAIR;
    return QG_MAP_QUAD;
}

// Which step kernels carry the fused observation pack (KPoLaunch): the one-link-per-lane kernel, and -- round 3 -- the four-wave-workgroup
// forms of the two-legs-per-lane and one-leg-per-lane kernels that AUTO runs above 4096 envs (explicit mapping requests on small
// grids, which launch the one-wave-workgroup forms, keep the observation pack a launch of its own).
bool qg_po_fusable(const qg_sim *s) {
    const int emap = qg_effective_mapping(s);
    if (emap == QG_MAP_LINK) return true;
    if (emap == QG_MAP_PAIR) return pair_wg4(s);
    if (emap == QG_MAP_QUAD) return quad_wg4(s);
    return false;
}

// A device-pointer step enqueued on a caller's stream: the next host-pointer call waits for the whole device, and from the first one
// that is CAPTURED on (sticky) every host-pointer call does.  (Not asked of the legacy NULL stream: while ANOTHER stream is in
// global-mode capture that query itself is a capture-implicit error and invalidates the capture in progress; a failed query counts
// as "captured" and its error is cleared.)
void qg_note_caller_stream(qg_sim *s, hipStream_t stream) {
    if (stream == s->stream) return;
    s->caller_inflight = 1;
    if (s->captured_once || !stream) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); s->captured_once = 1; }
    else if (cs == hipStreamCaptureStatusActive) s->captured_once = 1;
}

// `walk` != NULL: the fused walking launch (one-leg-per-lane kernel with the task layer folded in); walk_comps / walk_sample go
// with it
// `po` != NULL (with `walk`, one-link-per-lane mapping only): the partially observable observation pack fused in as well
int qg_launch_step(qg_sim *s, const float *d_actions, float *d_obs, float *d_reward, uint8_t *d_done, float *d_comps, float *d_packed,
                   hipStream_t stream, const KWalkLaunch *walk, const KPoLaunch *po) {
    KStepArgs P;
    P.st = s->st;
    P.n = s->n;
    P.track_ctrl = s->track_ctrl;
    P.actions = d_actions;
    P.obs = d_obs;
    P.reward = d_reward;
    P.done = d_done;
    P.comps = d_comps;
    P.packed = d_packed;
    P.seed = s->seed;
    P.env_index_base = s->env_index_base;
    const bool per_env = qg_sim_per_env(s);
    const StepLaunch L = {s, per_env ? &s->d_model_dyn->m : s->d_model, P, stream, walk, po};
    const int emap = qg_effective_mapping(s);
    if (s->res.launched) QG_TRY(qg_resident_retire(s));     // (the resident kernel holds the state in registers: it hands it back first)
    qg_note_caller_stream(s, stream);
    if (po && !(walk && qg_po_fusable(s))) return fail(QG_ERR_ARG, "launch_step: no step kernel with the fused observation pack for this handle");
    if (walk && emap == QG_MAP_LANE) return fail(QG_ERR_ARG, "launch_step: no step kernel with the fused walking task layer for this handle");
    const bool dyn_draw = s->task.auto_reset && (s->task.reset_flags & QG_RESET_DYNAMICS);
    if (dyn_draw && !s->dyn_range_set) return fail(QG_ERR_ARG, "step: task.reset_flags has QG_RESET_DYNAMICS and no range is set (qg_set_dynamics_range)");
    // per-env dynamics: the table-driven kernels' per-env forms, one link per lane up to 4096 envs (lagged sensors), one leg per lane
    // above (qg_set_mapping refuses the other mappings while the mode is on); wrench mode runs the same forms
    if (per_env && emap != QG_MAP_LINK && emap != QG_MAP_QUAD)
        return fail(QG_ERR_ARG, "step: per-env dynamics run in the LINK and QUAD mappings only (mapping %d)", emap);
    switch (emap) {                         // the leaves of a mapping are with its kernels (qg_step_launch.h)
    case QG_MAP_LINK: qg_select_step_link(L, per_env); break;
    case QG_MAP_QUAD: qg_select_step_quad(L, per_env); break;
    case QG_MAP_PAIR: qg_select_step_pair(L); break;
    default: qg_select_step_lane(L);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QG_ERR_LAUNCH, "qg_step_kernel launch: %s", hipGetErrorString(e));
    if (qg_jitter_at_reset(s)) {         // start-pose randomisation of the envs just auto-reset
        const int total = 12 * s->n, threads = 256;
        hipLaunchKernelGGL(qg_jitter_kernel, dim3((total + threads - 1) / threads), dim3(threads), 0, stream, s->d_model, s->d_task, s->st, s->n,
                           (const uint8_t *)d_done, (const float *)d_packed, s->obs_dim + 2, s->seed, s->env_index_base);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(QG_ERR_LAUNCH, "qg_jitter_kernel launch: %s", hipGetErrorString(e));
    }
    if (dyn_draw) {     // new dynamics rows of the envs just auto-reset, keyed as their reset yaw (episode - 1 after the increment)
        const int total = QG_NDYN * s->n, threads = 256;
        hipLaunchKernelGGL(qg_dyn_draw_kernel, dim3((total + threads - 1) / threads), dim3(threads), 0, stream, s->d_dyn, s->dyn_range,
                           (const int32_t *)s->st.episode, s->n, (const uint8_t *)nullptr, (const uint8_t *)d_done, (const float *)d_packed,
                           s->obs_dim + 2, -1, s->seed, s->env_index_base);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(QG_ERR_LAUNCH, "qg_dyn_draw_kernel launch: %s", hipGetErrorString(e));
    }
    return QG_OK;
}

extern "C" int qg_step_device(qg_sim *s, const float *actions, float *obs, float *reward, uint8_t *done, float *comps, void *stream) {
    if (!s || !actions || !obs || !reward || !done) return fail(QG_ERR_ARG, "qg_step_device: null argument");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    return qg_launch_step(s, actions, obs, reward, done, comps, nullptr, (hipStream_t)stream);
}

extern "C" int qg_step_device_packed(qg_sim *s, const float *actions, float *packed, void *stream) {
    if (!s || !actions || !packed) return fail(QG_ERR_ARG, "qg_step_device_packed: null argument");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    return qg_launch_step(s, actions, nullptr, nullptr, nullptr, nullptr, packed, (hipStream_t)stream);
}

// the two transposes on the library's stream, for the units that have no device code (qg_sim.h)
static int transpose_launch(qg_sim *s, void (*kernel)(const float *, float *, int, int), const float *src, float *dst, int w) {
    const int total = s->n * w, threads = 256;
    hipLaunchKernelGGL(kernel, dim3((total + threads - 1) / threads), dim3(threads), 0, s->stream, src, dst, s->n, w);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}
int qg_transpose_out_launch(qg_sim *s, const float *src, float *dst, int w) { return transpose_launch(s, qg_transpose_out, src, dst, w); }
int qg_transpose_in_launch(qg_sim *s, const float *src, float *dst, int w) { return transpose_launch(s, qg_transpose_in, src, dst, w); }

extern "C" int qg_time_step_kernel(qg_sim *s, const float *d_actions, float *d_packed, int32_t iters, float *ms_per_launch) {
    if (!s || !d_actions || !d_packed || iters < 1 || !ms_per_launch) return fail(QG_ERR_ARG, "qg_time_step_kernel: bad argument");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    QG_TRY(qg_retire_and_sync(s));
    // the launches are exactly what qg_step_device_packed enqueues (data.ctrl write-back as the handle has it set)
    HIP_TRY(hipEventRecord(s->ev0, s->stream), QG_ERR_DEVICE);
    for (int i = 0; i < iters; i++) QG_TRY(qg_launch_step(s, d_actions, nullptr, nullptr, nullptr, nullptr, d_packed, s->stream));
    HIP_TRY(hipEventRecord(s->ev1, s->stream), QG_ERR_DEVICE);
    HIP_TRY(hipEventSynchronize(s->ev1), QG_ERR_LAUNCH);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1), QG_ERR_DEVICE);
    *ms_per_launch = ms / (float)iters;
    return QG_OK;
}

extern "C" int qg_set_mapping(qg_sim *s, int32_t mapping) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if (mapping == QG_MAP_PAIR || mapping == QG_MAP_LANE)
        QG_TRY(qg_refuse_per_env(s, "qg_set_mapping: %s run in the LINK and QUAD mappings only (%s first)"));
    if (mapping == QG_MAP_PAIR && !qg_sim_baked(s))
        return fail(QG_ERR_ARG, "qg_set_mapping: the two-legs-per-lane kernel serves the compiled-in robot only");
    if (mapping != QG_MAP_AUTO && mapping != QG_MAP_LANE && mapping != QG_MAP_QUAD && mapping != QG_MAP_PAIR && mapping != QG_MAP_LINK)
        return fail(QG_ERR_ARG, "qg_set_mapping: unknown mapping %d", mapping);
    if (s->res.active) return fail(QG_ERR_ARG, "qg_set_mapping: the resident step mode is on (qg_resident_stop first)");
    s->mapping = mapping;
    return QG_OK;
}
extern "C" int qg_get_mapping(const qg_sim *s) { return s ? qg_effective_mapping(s) : fail(QG_ERR_ARG, "null handle"); }

/* 1 if the handle runs the kernel variant with the default robot's constants baked in as literals */
extern "C" int qg_uses_baked_model(const qg_sim *s) { return s ? qg_sim_baked(s) : fail(QG_ERR_ARG, "null handle"); }

extern "C" int qg_set_task(qg_sim *s, const qg_task *task) {
    if (!s || !task) return fail(QG_ERR_ARG, "qg_set_task: null argument");
    if (s->walk_bound) return fail(QG_ERR_ARG, "qg_set_task: a walking task layer is bound to this handle (it holds a copy of the task)");
    if (task->obs_mode != s->task.obs_mode) return fail(QG_ERR_ARG, "qg_set_task: obs_mode is fixed at qg_create (it sizes the output rows)");
    if (s->res.active) {              // the next ring relaunches the resident kernel: it has to be able to run the new task
        const qg_task old = s->task;
        s->task = *task;
        const int rc = qg_multi_step_usable(s, "the resident step mode");
        s->task = old;
        if (rc != QG_OK) {
            char why[256];
            snprintf(why, sizeof why, "%s", g_err);
            return fail(QG_ERR_ARG, "qg_set_task: %s (qg_resident_stop first)", why);
        }
    }
    KModel km;
    KTask kt;
    QG_TRY(build_tables(&s->model, task, &km, &kt));
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    QG_TRY(qg_retire_and_sync(s));   // steps reading the old task may be in flight on a caller's stream
    HIP_TRY(hipMemcpy(s->d_task, &kt, sizeof kt, hipMemcpyHostToDevice), QG_ERR_DEVICE);
    s->task = *task;
    return QG_OK;
}

extern "C" int qg_get_task(const qg_sim *s, qg_task *out) {
    if (!s || !out) return fail(QG_ERR_ARG, "qg_get_task: null argument");
    *out = s->task;
    return QG_OK;
}

extern "C" int32_t qg_debug_last_step_kernel(const qg_sim *s, char *buf, int32_t len) {
    if (!s || !buf || len < 1) return fail(QG_ERR_ARG, "qg_debug_last_step_kernel: bad argument");
    static const struct { const char *name; int nargs; } fam[] = {
        {nullptr, 0}, {"qg_step_kernel", 1}, {"qg_step_kernel_link", 5}, {"qg_step_kernel_quad", 7}, {"qg_step_kernel_pair", 3},
        {"qg_step_kernel_link_multi", 2}, {"qg_step_kernel_quad_multi", 2}, {"qg_step_kernel_pair_multi", 1}};
    const uint32_t code = s->last_step_kernel, f = code & 15u;
    if (f == KF_NONE || f > KF_PAIR_MULTI) return fail(QG_ERR_ARG, "qg_debug_last_step_kernel: no step kernel launched yet");
    char name[96];
    int k = snprintf(name, sizeof name, "%s<", fam[f].name);
    for (int a = 0; a < fam[f].nargs; a++) k += snprintf(name + k, sizeof name - k, a ? ",%u" : "%u", (code >> (4 + 4 * a)) & 15u);
    snprintf(name + k, sizeof name - k, ">");
    if ((int)strlen(name) >= len) return fail(QG_ERR_ARG, "qg_debug_last_step_kernel: need a buffer of %d bytes", (int)strlen(name) + 1);
    memcpy(buf, name, strlen(name) + 1);
    return QG_OK;
}

/* development builds (-DQG_PHASE_TIMES): the s_memrealtime stamps (10 ns units) of the last launch's first wave, read from the kernel
   unit that launched last (qg_step_launch.h); QG_ERR_ARG in production builds */
#ifdef QG_PHASE_TIMES
static QgPhaseReader g_phase_reader;
void qg_phase_unit(QgPhaseReader reader) { g_phase_reader = reader; }
#endif
extern "C" int qg_debug_phase_times(uint64_t out[16]) {
#ifdef QG_PHASE_TIMES
    if (!out) return fail(QG_ERR_ARG, "qg_debug_phase_times: null output");
    if (!g_phase_reader) return fail(QG_ERR_ARG, "qg_debug_phase_times: no step kernel launched yet");
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    HIP_TRY(g_phase_reader(out), QG_ERR_DEVICE);
    return QG_OK;
#else
    (void)out;
    return fail(QG_ERR_ARG, "qg_debug_phase_times: the library was built without -DQG_PHASE_TIMES");
#endif
}

extern "C" int qg_set_track_ctrl(qg_sim *s, int32_t on) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if ((on ? 1 : 0) != s->track_ctrl) QG_TRY(qg_resident_retire(s));      // (a resident launch holds the old setting)
    s->track_ctrl = on ? 1 : 0;
    return QG_OK;
}

// the reset streams of the simulator itself: the per-env episode counters and the batch seed that key every random draw of a
// (re)set -- what qg_get_state does not cover and a bit-exact resume under auto-reset needs
extern "C" int qg_get_reset_streams(qg_sim *s, int32_t *episode, uint64_t *seed) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    QG_TRY(qg_retire_and_sync(s));
    if (episode) HIP_TRY(hipMemcpy(episode, s->st.episode, (size_t)s->n * sizeof(int32_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    if (seed) *seed = s->seed;
    return QG_OK;
}
extern "C" int qg_set_reset_streams(qg_sim *s, const int32_t *episode, uint64_t seed) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    QG_TRY(qg_retire_and_sync(s));
    if (episode) HIP_TRY(hipMemcpy(s->st.episode, episode, (size_t)s->n * sizeof(int32_t), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    s->seed = seed;
    return QG_OK;
}
