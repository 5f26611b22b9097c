// qg_capi.hip -- the core of the C ABI declared in include/quadgym.h: the simulator handle.
//
// Owns the per-env device state (struct-of-arrays in HBM), converts the double-precision
// model/task descriptions into the kernarg-sized single-precision tables the kernels read,
// and decides which mapping a step runs.  The step kernels, their launchers and the leaves of each mapping are translation units of
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

static int resident_retire(qg_sim *s);
static void resident_free(qg_sim *s);
static int multi_step_usable(const qg_sim *s, const char *who);

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
    int rc = resident_retire(s);
    if (rc != QG_OK) return rc;
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_destroy(qg_sim *s) {
    if (!s) return QG_OK;
    (void)hipSetDevice(s->device);
    (void)resident_retire(s);
    (void)hipDeviceSynchronize();                  // steps may still be in flight on a caller's stream (the header's ordering contract)
    resident_free(s);
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
    int rc = build_tables(model, task, &km, &kt);
    if (rc != QG_OK) return rc;

    int simds;
    if ((rc = qg_open_device(device_id, &simds)) != QG_OK) return rc;

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
        s->baked = QG_BAKED_LEGS_IDENTICAL && memcmp(&km, &baked, sizeof km) == 0;
        s->model_baked = s->baked;
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
    rc = qg_reset(s, nullptr, 0, 0);
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
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }
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
    if (s->mapping == QG_MAP_PAIR) return s->baked ? QG_MAP_PAIR : QG_MAP_QUAD;
    // (the one-link-per-lane kernel addresses the state with 32-bit byte offsets from scalar bases: 19 n floats must stay below 4 GiB)
    if (s->mapping == QG_MAP_LINK) return (s->task.sensor_lag && s->n <= (1 << 24)) ? QG_MAP_LINK : QG_MAP_QUAD;
    // up to one wave of the one-link-per-lane kernel per SIMD (4096 envs on the 1024 SIMDs of an MI355X); the other boundaries are
    // the same measurement in units of "waves per SIMD" (pair: > 1 quad wave per SIMD up to 1 pair wave per SIMD, and from 1.75 on)
    const int simds = s->simds;
    if (s->task.sensor_lag && s->n <= simds * QGK_LINK_ENVS) return QG_MAP_LINK;
    if (s->baked && s->n > simds * QGK_QUAD_ENVS && (s->n <= simds * QGK_PAIR_ENVS || s->n >= (simds + 3 * (simds / 4)) * QGK_PAIR_ENVS)) return QG_MAP_PAIR;
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

static bool jitter_at_reset(const qg_sim *s) { return s->task.auto_reset && (s->task.reset_flags & QG_RESET_JOINT_JITTER); }

// A device-pointer step enqueued on a caller's stream: the next host-pointer call waits for the whole device, and from the first one
// that is CAPTURED on (sticky) every host-pointer call does.  (Not asked of the legacy NULL stream: while ANOTHER stream is in
// global-mode capture that query itself is a capture-implicit error and invalidates the capture in progress; a failed query counts
// as "captured" and its error is cleared.)
static void note_caller_stream(qg_sim *s, hipStream_t stream) {
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
    const bool per_env = s->dyn || s->xfrc;
    const StepLaunch L = {s, per_env ? &s->d_model_dyn->m : s->d_model, P, stream, walk, po};
    const int emap = qg_effective_mapping(s);
    if (s->res.launched) {            // a per-launch step while the resident kernel holds the state in registers: it has to hand it back first
        int rr = resident_retire(s);
        if (rr != QG_OK) return rr;
    }
    note_caller_stream(s, stream);
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
    if (jitter_at_reset(s)) {         // start-pose randomisation of the envs just auto-reset
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

// ---- page-locked staging of the host-pointer entry points --------------------------------------------------------------------------
// The caller's buffers are ordinary (pageable) memory: a hipMemcpyAsync from / to them is a synchronous, staged copy with ~10-15 us of
// fixed cost each -- five of them made a ONE-env qg_step 70 us for a 10 us kernel.  The entry points therefore copy through one
// page-locked arena per handle: host memcpy in, truly asynchronous transfers enqueued around the launch, one stream synchronisation,
// host memcpy out (tools/host_step_rate.py).
static int pin_reserve(qg_sim *s, size_t bytes) {
    if (bytes <= s->h_pin_cap) return QG_OK;
    if (s->h_pin) { (void)hipHostFree(s->h_pin); s->h_pin = nullptr; s->h_pin_cap = 0; }
    size_t cap = bytes + bytes / 4 + 4096;
    HIP_TRY(hipHostMalloc((void **)&s->h_pin, cap, hipHostMallocDefault), QG_ERR_ALLOC);
    s->h_pin_cap = cap;
    return QG_OK;
}
static size_t pin_align(size_t x) { return (x + 255) & ~(size_t)255; }
// actions (host) -> device through the arena's first bytes, asynchronously on the library's stream
static int pin_actions_in(qg_sim *s, const float *actions, float *d_actions) {
    const size_t bytes = (size_t)s->n * QG_NU * sizeof(float);
    memcpy(s->h_pin, actions, bytes);
    HIP_TRY(hipMemcpyAsync(d_actions, s->h_pin, bytes, hipMemcpyHostToDevice, s->stream), QG_ERR_DEVICE);
    return QG_OK;
}
// Above ~1 MB the detour loses: the extra host copy into the caller's (often freshly allocated, not yet touched) array costs more than
// the staged transfer's fixed overhead -- the 4.3 MB observation stack of 4096 partially observable envs went from 213 to 369 us per step
// through the arena -- so large outputs go straight to the caller's memory.
#define QG_PIN_MAX_BYTES ((size_t)1 << 20)
static int pin_out_enqueue(qg_sim *s, const PinOut &o, const void *d_src) {
    if (!o.user) return QG_OK;
    void *dst = o.bytes > QG_PIN_MAX_BYTES ? o.user : (void *)(s->h_pin + o.off);
    HIP_TRY(hipMemcpyAsync(dst, d_src, o.bytes, hipMemcpyDeviceToHost, s->stream), QG_ERR_DEVICE);
    return QG_OK;
}
static void pin_out_finish(qg_sim *s, const PinOut &o) {
    if (o.user && o.bytes <= QG_PIN_MAX_BYTES) memcpy(o.user, s->h_pin + o.off, o.bytes);
}

// The host-pointer steps must not overtake device-pointer steps still in flight on a caller's stream; a device-wide wait is only
// needed if one has been enqueued since the last one (the library's own stream is synchronised at the end of every host-pointer call).
static int wait_for_caller_streams(qg_sim *s) {
    { int rr = resident_retire(s); if (rr != QG_OK) return rr; }
    if (!s->caller_inflight && !s->captured_once) return QG_OK;
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    s->caller_inflight = 0;
    return QG_OK;
}

static int copy_in(qg_sim *s, const float *host, float *field_major, int w) {
    if (!host) return QG_OK;
    int total = s->n * w, threads = 256;
    HIP_TRY(hipMemcpyAsync(s->d_stage, host, (size_t)total * sizeof(float), hipMemcpyHostToDevice, s->stream), QG_ERR_DEVICE);
    hipLaunchKernelGGL(qg_transpose_in, dim3((total + threads - 1) / threads), dim3(threads), 0, s->stream, s->d_stage, field_major, s->n, w);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    HIP_TRY(hipStreamSynchronize(s->stream), QG_ERR_LAUNCH);
    return QG_OK;
}

int qg_transpose_out_launch(qg_sim *s, const float *src, float *dst, int w) {
    const int total = s->n * w, threads = 256;
    hipLaunchKernelGGL(qg_transpose_out, dim3((total + threads - 1) / threads), dim3(threads), 0, s->stream, src, dst, s->n, w);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

// State snapshot, part 1: where the five outputs land in the page-locked arena (from `off` on); part 2: the four transposes into their
// own regions of the staging buffer and every transfer, enqueued on the library's stream (no synchronisation in here).
static size_t state_out_layout(qg_sim *s, const StateDst &d, size_t off, PinOut (&so)[5]) {
    const size_t n = (size_t)s->n;
    float *dst[4] = {d.qpos, d.qvel, d.act, d.ctrl};
    const int w[4] = {QG_NQ, QG_NV, QG_NU, QG_NU};
    for (int f = 0; f < 4; f++) { so[f] = {dst[f], off, n * w[f] * sizeof(float)}; off += pin_align(so[f].bytes); }
    so[4] = {d.nstep, off, n * sizeof(int32_t)};
    return off + pin_align(so[4].bytes);
}
static int state_out_enqueue(qg_sim *s, const PinOut (&so)[5]) {
    const size_t n = (size_t)s->n;
    const float *src[4] = {s->st.qpos, s->st.qvel, s->st.act, s->st.ctrl};
    const int w[4] = {QG_NQ, QG_NV, QG_NU, QG_NU};
    size_t soff = 0;
    int rc;
    for (int f = 0; f < 4; f++) {
        float *stage = s->d_stage + soff;
        soff += n * w[f];
        if (!so[f].user) continue;
        if ((rc = qg_transpose_out_launch(s, src[f], stage, w[f])) != QG_OK) return rc;
        if ((rc = pin_out_enqueue(s, so[f], stage)) != QG_OK) return rc;
    }
    return pin_out_enqueue(s, so[4], s->st.nstep);
}

extern "C" int qg_get_state(qg_sim *s, float *qpos, float *qvel, float *act, float *ctrl, int32_t *nstep) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }   // steps may be in flight on a caller's stream
    // every transfer enqueued, ONE synchronisation (five synchronised round trips made the single-env facade's mirror of the state
    // 120 us of a 160 us step)
    PinOut so[5];
    int rc = pin_reserve(s, state_out_layout(s, {qpos, qvel, act, ctrl, nstep}, 0, so));
    if (rc == QG_OK) rc = state_out_enqueue(s, so);
    if (rc != QG_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream), QG_ERR_LAUNCH);
    for (int f = 0; f < 5; f++) pin_out_finish(s, so[f]);
    return QG_OK;
}

// the two halves of host_step (qg_sim.h) around the step's own launch
int qg_host_step_begin(qg_sim *s, const float *actions, float *d_actions, const HostOut (&out)[4], const StateDst *state, HostStep &h) {
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    { int rc0 = wait_for_caller_streams(s); if (rc0 != QG_OK) return rc0; }
    size_t off = pin_align((size_t)s->n * QG_NU * sizeof(float));
    for (int i = 0; i < 4; i++) { h.o[i] = {out[i].user, off, out[i].bytes}; off += pin_align(h.o[i].bytes); }
    if (state) off = state_out_layout(s, *state, off, h.state);
    int rc = pin_reserve(s, off);
    if (rc == QG_OK) rc = pin_actions_in(s, actions, d_actions);
    return rc;
}
int qg_host_step_end(qg_sim *s, const HostOut (&out)[4], const StateDst *state, const HostStep &h) {
    int rc = QG_OK;
    for (int i = 0; i < 4 && rc == QG_OK; i++) rc = pin_out_enqueue(s, h.o[i], out[i].dev);
    if (rc == QG_OK && state) rc = state_out_enqueue(s, h.state);
    if (rc != QG_OK) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream), QG_ERR_LAUNCH);
    for (int i = 0; i < 4; i++) pin_out_finish(s, h.o[i]);
    if (state)
        for (int f = 0; f < 5; f++) pin_out_finish(s, h.state[f]);
    return QG_OK;
}
static int sim_host_step(qg_sim *s, const float *actions, float *obs, float *reward, uint8_t *done, float *comps, const StateDst *state) {
    const size_t n = (size_t)s->n;
    const HostOut out[4] = {{obs, s->d_obs, n * s->obs_dim * sizeof(float)}, {reward, s->d_reward, n * sizeof(float)}, {done, s->d_done, n},
                            {comps, s->d_comps, n * QG_NREWARD * sizeof(float)}};
    return host_step(s, actions, s->d_actions, out, [&] {
        return qg_launch_step(s, s->d_actions, s->d_obs, s->d_reward, s->d_done, comps ? s->d_comps : nullptr, nullptr, s->stream);
    }, state);
}

extern "C" int qg_step(qg_sim *s, const float *actions, float *obs, float *reward, uint8_t *done, float *comps) {
    if (!s || !actions || !obs || !reward || !done) return fail(QG_ERR_ARG, "qg_step: null argument");
    return sim_host_step(s, actions, obs, reward, done, comps, nullptr);
}

// qg_step and qg_get_state in one call and one synchronisation: what an env that mirrors the state on the host after every step
// (the reference's `env.data`, read by user reward / termination callables) needs.
extern "C" int qg_step_mirror(qg_sim *s, const float *actions, float *obs, float *reward, uint8_t *done, float *comps, float *qpos, float *qvel,
                              float *act, float *ctrl, int32_t *nstep) {
    if (!s || !actions || !obs || !reward || !done) return fail(QG_ERR_ARG, "qg_step_mirror: null argument");
    const StateDst state = {qpos, qvel, act, ctrl, nstep};
    return sim_host_step(s, actions, obs, reward, done, comps, &state);
}

extern "C" int qg_set_state(qg_sim *s, const float *qpos, const float *qvel, const float *act, const float *ctrl, const int32_t *nstep) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }
    int rc;
    if ((rc = copy_in(s, qpos, s->st.qpos, QG_NQ)) != QG_OK) return rc;
    if ((rc = copy_in(s, qvel, s->st.qvel, QG_NV)) != QG_OK) return rc;
    if ((rc = copy_in(s, act, s->st.act, QG_NU)) != QG_OK) return rc;
    if ((rc = copy_in(s, ctrl, s->st.ctrl, QG_NU)) != QG_OK) return rc;
    if (nstep) HIP_TRY(hipMemcpy(s->st.nstep, nstep, (size_t)s->n * sizeof(int32_t), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    return QG_OK;
}

extern "C" int qg_time_step_kernel(qg_sim *s, const float *d_actions, float *d_packed, int32_t iters, float *ms_per_launch) {
    if (!s || !d_actions || !d_packed || iters < 1 || !ms_per_launch) return fail(QG_ERR_ARG, "qg_time_step_kernel: bad argument");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }
    // the launches are exactly what qg_step_device_packed enqueues (data.ctrl write-back as the handle has it set)
    HIP_TRY(hipEventRecord(s->ev0, s->stream), QG_ERR_DEVICE);
    for (int i = 0; i < iters; i++) {
        int rc = qg_launch_step(s, d_actions, nullptr, nullptr, nullptr, nullptr, d_packed, s->stream);
        if (rc != QG_OK) return rc;
    }
    HIP_TRY(hipEventRecord(s->ev1, s->stream), QG_ERR_DEVICE);
    HIP_TRY(hipEventSynchronize(s->ev1), QG_ERR_LAUNCH);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1), QG_ERR_DEVICE);
    *ms_per_launch = ms / (float)iters;
    return QG_OK;
}

extern "C" int qg_set_mapping(qg_sim *s, int32_t mapping) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if (s->dyn && (mapping == QG_MAP_PAIR || mapping == QG_MAP_LANE))
        return fail(QG_ERR_ARG, "qg_set_mapping: per-env dynamics run in the LINK and QUAD mappings only (qg_clear_dynamics first)");
    if (s->xfrc && (mapping == QG_MAP_PAIR || mapping == QG_MAP_LANE))
        return fail(QG_ERR_ARG, "qg_set_mapping: external wrenches run in the LINK and QUAD mappings only (qg_clear_xfrc first)");
    if (mapping == QG_MAP_PAIR && !s->baked)
        return fail(QG_ERR_ARG, "qg_set_mapping: the two-legs-per-lane kernel serves the compiled-in robot only");
    if (mapping != QG_MAP_AUTO && mapping != QG_MAP_LANE && mapping != QG_MAP_QUAD && mapping != QG_MAP_PAIR && mapping != QG_MAP_LINK)
        return fail(QG_ERR_ARG, "qg_set_mapping: unknown mapping %d", mapping);
    if (s->res.active) return fail(QG_ERR_ARG, "qg_set_mapping: the resident step mode is on (qg_resident_stop first)");
    s->mapping = mapping;
    return QG_OK;
}
extern "C" int qg_get_mapping(const qg_sim *s) { return s ? qg_effective_mapping(s) : fail(QG_ERR_ARG, "null handle"); }

/* 1 if the handle runs the kernel variant with the default robot's constants baked in as literals */
extern "C" int qg_uses_baked_model(const qg_sim *s) { return s ? s->baked : fail(QG_ERR_ARG, "null handle"); }

extern "C" int qg_set_task(qg_sim *s, const qg_task *task) {
    if (!s || !task) return fail(QG_ERR_ARG, "qg_set_task: null argument");
    if (s->walk_bound) return fail(QG_ERR_ARG, "qg_set_task: a walking task layer is bound to this handle (it holds a copy of the task)");
    if (task->obs_mode != s->task.obs_mode) return fail(QG_ERR_ARG, "qg_set_task: obs_mode is fixed at qg_create (it sizes the output rows)");
    if (s->res.active) {              // the next ring relaunches the resident kernel: it has to be able to run the new task
        const qg_task old = s->task;
        s->task = *task;
        const int rc = multi_step_usable(s, "the resident step mode");
        s->task = old;
        if (rc != QG_OK) {
            char why[256];
            snprintf(why, sizeof why, "%s", g_err);
            return fail(QG_ERR_ARG, "qg_set_task: %s (qg_resident_stop first)", why);
        }
    }
    KModel km;
    KTask kt;
    int rc = build_tables(&s->model, task, &km, &kt);
    if (rc != QG_OK) return rc;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }   // steps reading the old task may be in flight on a caller's stream
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
    if ((on ? 1 : 0) != s->track_ctrl) { int rr = resident_retire(s); if (rr != QG_OK) return rr; }      // (a resident launch holds the old setting)
    s->track_ctrl = on ? 1 : 0;
    return QG_OK;
}

// ------------------------------------------------------------------------------------------------------
// many env-steps per launch: the sequence forms, and the resident form of the one-link-per-lane kernel (qg_kernel_resident.hip)
// ------------------------------------------------------------------------------------------------------
static int multi_step_usable(const qg_sim *s, const char *who) {
    if (qg_effective_mapping(s) != QG_MAP_LINK)
        return fail(QG_ERR_ARG, "%s: needs the one-link-per-lane mapping (AUTO up to 4096 envs, lagged sensors)", who);
    if (s->n > s->simds * QGK_LINK_ENVS) return fail(QG_ERR_ARG, "%s: at most %d envs (one wave per SIMD)", who, s->simds * QGK_LINK_ENVS);
    if (s->walk_bound) return fail(QG_ERR_ARG, "%s: a walking task layer is bound to this handle", who);
    if (jitter_at_reset(s))
        return fail(QG_ERR_ARG, "%s: hinge jitter at auto-reset is a launch of its own behind every step; not available in this form", who);
    return QG_OK;
}
static KStepArgs multi_step_args(const qg_sim *s) {
    KStepArgs P = {};
    P.st = s->st;
    P.n = s->n;
    P.track_ctrl = s->track_ctrl;
    P.seed = s->seed;
    P.env_index_base = s->env_index_base;
    return P;
}
extern "C" int qg_step_device_seq(qg_sim *s, const float *actions, float *packed, int32_t count, void *stream) {
    if (!s || !actions || !packed || count < 1) return fail(QG_ERR_ARG, "qg_step_device_seq: bad argument");
    if (s->dyn) return fail(QG_ERR_ARG, "qg_step_device_seq: not available with per-env dynamics (qg_clear_dynamics first)");
    if (s->xfrc) return fail(QG_ERR_ARG, "qg_step_device_seq: not available with external wrenches (qg_clear_xfrc first)");
    if (s->walk_bound) return fail(QG_ERR_ARG, "qg_step_device_seq: a walking task layer is bound to this handle");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    int rc;
    if (s->res.launched && (rc = resident_retire(s)) != QG_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int emap = qg_effective_mapping(s);
    // the two-legs-per-lane mapping (16 385 .. 32 768 envs, >= 57 344) and the one-leg-per-lane mapping on the grids AUTO gives it
    // (four-wave workgroups) have one-launch forms of their own
    const bool seq_pair = emap == QG_MAP_PAIR && s->baked && s->task.sensor_lag && !jitter_at_reset(s);
    const bool seq_quad = emap == QG_MAP_QUAD && s->task.sensor_lag && quad_wg4(s) && !jitter_at_reset(s);
    if (!seq_pair && !seq_quad && multi_step_usable(s, "qg_step_device_seq") != QG_OK) {
        // another mapping (more than one wave per SIMD of the one-link-per-lane kernel), or hinge jitter behind every step: the same
        // rows from `count` per-step launches -- the call means the same thing for every handle, the one-launch form is the fast path
        const size_t arow = (size_t)s->n * QG_NU, prow = (size_t)s->n * (s->obs_dim + 2);
        for (int32_t k = 0; k < count; k++)
            if ((rc = qg_launch_step(s, actions + k * arow, nullptr, nullptr, nullptr, nullptr, packed + k * prow, st)) != QG_OK) return rc;
        return QG_OK;
    }
    note_caller_stream(s, st);
    KResident R = {};
    R.actions = actions;
    R.packed = packed;
    R.count = count;
    R.slots = 1;
    const KStepArgs P = multi_step_args(s);
    if (seq_pair) qg_select_seq_pair(s, st, P, R);
    else if (seq_quad) qg_select_seq_quad(s, st, P, R);
    else qg_select_seq_link(s, st, P, R);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QG_ERR_LAUNCH, "qg_step_device_seq launch: %s", hipGetErrorString(e));
    return QG_OK;
}

static void resident_free(qg_sim *s) {
    if (s->res.d_mail) (void)hipFree(s->res.d_mail);
    if (s->res.own_buffers && s->res.k.actions) (void)hipFree((void *)s->res.k.actions);
    if (s->res.own_buffers && s->res.k.packed) (void)hipFree(s->res.k.packed);
    if (s->res.hstat) (void)hipHostFree((void *)s->res.hstat);
    if (s->res.ctl_stream) (void)hipStreamDestroy(s->res.ctl_stream);
    memset(&s->res, 0, sizeof s->res);
}

// The resident kernel stores the state it holds in registers and leaves: STOP into the door (the waves first finish what has been
// rung), then the library's stream -- where the kernel runs -- is waited for.  Rings still queued on the caller's stream are waited
// for first, so that "every step enqueued before this call" has run, as the ordering contract of quadgym.h says.
static int resident_retire(qg_sim *s) {
    if (!s->res.active || !s->res.launched) return QG_OK;
    if (s->res.last_stream) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s->res.last_stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusActive)
            return fail(QG_ERR_ARG, "the resident step kernel cannot be retired while its rings are being captured");
        (void)hipStreamSynchronize(s->res.last_stream);      // (a stream the caller has destroyed since is no reason to fail)
        (void)hipGetLastError();
    }
    qg_launch_resident_ctl(s->res.ctl_stream, s->res.k.door, 0);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    HIP_TRY(hipStreamSynchronize(s->res.ctl_stream), QG_ERR_LAUNCH);
    HIP_TRY(hipStreamSynchronize(s->stream), QG_ERR_LAUNCH);
    s->res.launched = 0;
    return QG_OK;
}

// (re)launch on the library's stream: clear STOP, then the kernel; it starts at the env-step the previous launch left off at
static int resident_launch(qg_sim *s) {
    int rc = multi_step_usable(s, "resident kernel launch");
    if (rc != QG_OK) return rc;
    s->res.hstat[0] = QG_RES_RUNNING;
    qg_launch_resident_ctl(s->stream, s->res.k.door, 1);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    qg_select_resident(s, multi_step_args(s));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QG_ERR_LAUNCH, "resident kernel launch: %s", hipGetErrorString(e));
    s->res.launched = 1;
    // (a ring on another stream that gets to the door before the two launches above sees STOP with `RUNNING` in hstat and waits for
    // the door to open -- qg_resident_ring_kernel -- so nothing has to be waited for here)
    return QG_OK;
}

extern "C" int qg_resident_start(qg_sim *s, int32_t slots, int32_t idle_timeout_us, float *actions, float *packed) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if ((actions == nullptr) != (packed == nullptr)) return fail(QG_ERR_ARG, "qg_resident_start: pass both slot buffers or neither");
    if (s->res.active) return fail(QG_ERR_ARG, "qg_resident_start: already on");
    if (s->dyn) return fail(QG_ERR_ARG, "qg_resident_start: not available with per-env dynamics (qg_clear_dynamics first)");
    if (s->xfrc) return fail(QG_ERR_ARG, "qg_resident_start: not available with external wrenches (qg_clear_xfrc first)");
    if (slots < 1 || slots > 4096) return fail(QG_ERR_ARG, "qg_resident_start: slots must be 1..4096");
    if (idle_timeout_us == 0) idle_timeout_us = 2000;
    if (idle_timeout_us < 50 || idle_timeout_us > 100000) return fail(QG_ERR_ARG, "qg_resident_start: idle_timeout_us must be 50..100000 (0 = 2000)");
    int rc = multi_step_usable(s, "qg_resident_start");
    if (rc != QG_OK) return rc;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    const size_t n = (size_t)s->n, row = (size_t)s->obs_dim + 2;
    const size_t mail_bytes = 256 + QG_RES_SHARDS * 128 + 256;
    hipError_t e = hipMalloc(&s->res.d_mail, mail_bytes);
    if (e == hipSuccess) e = hipMemset(s->res.d_mail, 0, mail_bytes);
    s->res.own_buffers = actions == nullptr;
    if (s->res.own_buffers) {
        float *acts = nullptr;
        if (e == hipSuccess) e = hipMalloc((void **)&acts, (size_t)slots * n * QG_NU * sizeof(float));
        if (e == hipSuccess) e = hipMemset(acts, 0, (size_t)slots * n * QG_NU * sizeof(float));
        s->res.k.actions = acts;
        if (e == hipSuccess) e = hipMalloc((void **)&s->res.k.packed, (size_t)slots * n * row * sizeof(float));
        if (e == hipSuccess) e = hipMemset(s->res.k.packed, 0, (size_t)slots * n * row * sizeof(float));
    } else {
        s->res.k.actions = actions;
        s->res.k.packed = packed;
    }
    if (e == hipSuccess) e = hipHostMalloc((void **)&s->res.hstat, 64, hipHostMallocCoherent | hipHostMallocMapped);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->res.ctl_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        resident_free(s);
        return fail(QG_ERR_ALLOC, "qg_resident_start: %s", hipGetErrorString(e));
    }
    for (int i = 0; i < 8; i++) s->res.hstat[i] = 0;
    uint8_t *m = (uint8_t *)s->res.d_mail;
    s->res.k.door = (unsigned long long *)m;
    s->res.k.done = (unsigned long long *)(m + 256);
    s->res.k.completed = (unsigned long long *)(m + 256 + QG_RES_SHARDS * 128);
    s->res.k.hstat = (unsigned long long *)s->res.hstat;
    s->res.k.slots = slots;
    s->res.k.count = 0;
    s->res.k.idle_ticks = (uint32_t)idle_timeout_us * 100u;
    s->res.k.ring_ticks = 20000000u;          // 200 ms without a single arrival: the ring gives up and says so
    s->res.active = 1;
    s->res.rung = 0;
    return resident_launch(s);
}

extern "C" int qg_resident_stop(qg_sim *s) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if (!s->res.active) return QG_OK;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    int rc = qg_retire_and_sync(s);
    if (rc != QG_OK) return rc;
    resident_free(s);
    return QG_OK;
}

extern "C" int qg_resident_buffers(qg_sim *s, float **actions, float **packed, int32_t *slots) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if (!s->res.active) return fail(QG_ERR_ARG, "qg_resident_buffers: the resident step mode is off");
    if (actions) *actions = (float *)s->res.k.actions;
    if (packed) *packed = s->res.k.packed;
    if (slots) *slots = s->res.k.slots;
    return QG_OK;
}

// rings that found the kernel retired, or gave up waiting, since the last look: an error the caller must see once
static int resident_check_reports(qg_sim *s, const char *who) {
    const uint64_t lost = s->res.hstat[2], gave = s->res.hstat[3];
    if (lost != s->res.lost_seen) {
        const uint64_t d = lost - s->res.lost_seen;
        s->res.lost_seen = lost;
        s->res.rung -= (int64_t)d;        // those rings did not advance the door: the count (and the slot of the next env-step) follows the device
        return fail(QG_ERR_LAUNCH, "%s: %llu env-step(s) were rung after the resident kernel had retired and were NOT executed "
                    "(rings must follow one another within the idle time-out, or call qg_resident_ensure before a burst)", who, (unsigned long long)d);
    }
    if (gave != s->res.gaveup_seen) {
        s->res.gaveup_seen = gave;
        return fail(QG_ERR_LAUNCH, "%s: a ring gave up waiting for the resident kernel (no arrival for 200 ms)", who);
    }
    return QG_OK;
}

extern "C" int qg_resident_ensure(qg_sim *s) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if (!s->res.active) return fail(QG_ERR_ARG, "qg_resident_ensure: the resident step mode is off");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    if (s->res.launched && s->res.hstat[0] == QG_RES_RUNNING) return QG_OK;
    if (s->res.launched && s->res.hstat[0] == QG_RES_RETIRING) {
        // no ring for half the time-out: the kernel may shut the door before a ring enqueued now reaches it.  Retire it here (it
        // stores the state and leaves within microseconds) and launch it again: a fresh idle clock for what follows.
        int rc = resident_retire(s);
        if (rc != QG_OK) return rc;
    }
    return resident_launch(s);        // stream-ordered behind the launch that has left (or is leaving)
}

extern "C" int qg_resident_step_device(qg_sim *s, int32_t count, void *stream) {
    if (!s || count < 1) return fail(QG_ERR_ARG, "qg_resident_step_device: bad argument");
    if (!s->res.active) return fail(QG_ERR_ARG, "qg_resident_step_device: the resident step mode is off (qg_resident_start)");
    if (count > s->res.k.slots) return fail(QG_ERR_ARG, "qg_resident_step_device: count %d exceeds the %d slots of the mailbox", count, s->res.k.slots);
    if ((hipStream_t)stream == s->stream) return fail(QG_ERR_ARG, "qg_resident_step_device: that is the stream the resident kernel occupies");
    int rc = resident_check_reports(s, "qg_resident_step_device");
    if (rc != QG_OK) return rc;
    if ((rc = qg_resident_ensure(s)) != QG_OK) return rc;
    const unsigned nwaves = link_blocks(s) * QGK_LINK_WAVES;
    qg_launch_resident_ring((hipStream_t)stream, s->res.k, (unsigned)count, nwaves, (unsigned long long)s->res.rung);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(QG_ERR_LAUNCH, "ring kernel launch: %s", hipGetErrorString(e));
    s->res.last_stream = (hipStream_t)stream;
    s->res.rung += count;
    return QG_OK;
}

extern "C" int qg_resident_status(qg_sim *s, int64_t *rung, int32_t *running, int64_t *completed_at_exit, int64_t *not_executed) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if (!s->res.active) return fail(QG_ERR_ARG, "qg_resident_status: the resident step mode is off");
    if (rung) *rung = s->res.rung;
    if (running) *running = s->res.launched && s->res.hstat[0] == QG_RES_RUNNING;
    if (completed_at_exit) *completed_at_exit = (int64_t)s->res.hstat[1];
    if (not_executed) *not_executed = (int64_t)s->res.hstat[2];
    return QG_OK;
}

// the reset streams of the simulator itself: the per-env episode counters and the batch seed that key every random draw of a
// (re)set -- what qg_get_state does not cover and a bit-exact resume under auto-reset needs
extern "C" int qg_get_reset_streams(qg_sim *s, int32_t *episode, uint64_t *seed) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }
    if (episode) HIP_TRY(hipMemcpy(episode, s->st.episode, (size_t)s->n * sizeof(int32_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    if (seed) *seed = s->seed;
    return QG_OK;
}
extern "C" int qg_set_reset_streams(qg_sim *s, const int32_t *episode, uint64_t seed) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }
    if (episode) HIP_TRY(hipMemcpy(s->st.episode, episode, (size_t)s->n * sizeof(int32_t), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    s->seed = seed;
    return QG_OK;
}

// ------------------------------------------------------------------------------------------------------
// per-env dynamics (include/quadgym.h, QG_NDYN columns)
// ------------------------------------------------------------------------------------------------------
static void dyn_identity_row(const qg_sim *s, float row[QG_NDYN]) {
    for (int c = 0; c < QG_NDYN; c++) row[c] = 1.f;
    row[QG_DYN_FRICTION] = (float)s->model.contact_friction;
    row[QG_DYN_PAYLOAD_MASS] = row[QG_DYN_PAYLOAD_X] = row[QG_DYN_PAYLOAD_Y] = row[QG_DYN_PAYLOAD_Z] = 0.f;
}
// one row against the model: finite, friction and scales >= 0, FRAME mass > 0, rotational inertia about the new centre of mass positive
// definite (f64; what the payload does to the FRAME's rigid inertia, the same rule as the kernels' dyn_load)
static int dyn_check_row(const qg_sim *s, const float *row, const char *who, const char *what) {
    for (int c = 0; c < QG_NDYN; c++) {      // (exponent bits: the device pass, which parses this too, assumes finite math)
        uint32_t bits;
        memcpy(&bits, row + c, 4);
        if (((bits >> 23) & 0xFFu) == 0xFFu) return fail(QG_ERR_ARG, "%s: %s: column %d is not finite", who, what, c);
    }
    if (row[QG_DYN_FRICTION] < 0) return fail(QG_ERR_ARG, "%s: %s: friction %g < 0", who, what, (double)row[QG_DYN_FRICTION]);
    for (int c = QG_DYN_KP_SCALE; c < QG_NDYN; c++)
        if (row[c] < 0) return fail(QG_ERR_ARG, "%s: %s: scale column %d is %g < 0", who, what, c, (double)row[c]);
    const qg_model &m = s->model;
    const double dm = row[QG_DYN_PAYLOAD_MASS], p[3] = {row[QG_DYN_PAYLOAD_X], row[QG_DYN_PAYLOAD_Y], row[QG_DYN_PAYLOAD_Z]};
    const double m1 = m.body_mass[0] + dm;
    if (!(m1 > 0)) return fail(QG_ERR_ARG, "%s: %s: FRAME mass %g + payload %g <= 0", who, what, m.body_mass[0], dm);
    // about the FRAME origin: body inertia (about its COM) shifted there, plus the point mass
    const double *c0 = m.body_ipos[0], *I = m.body_inertia[0], m0 = m.body_mass[0];
    double J[3][3] = {{I[0], I[3], I[4]}, {I[3], I[1], I[5]}, {I[4], I[5], I[2]}};
    const double cc = c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2], pp = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    double h[3];
    for (int a = 0; a < 3; a++) {
        h[a] = m0 * c0[a] + dm * p[a];
        for (int b = 0; b < 3; b++) J[a][b] += m0 * ((a == b ? cc : 0) - c0[a] * c0[b]) + dm * ((a == b ? pp : 0) - p[a] * p[b]);
    }
    // back to the new centre of mass c1 = h / m1
    const double c1[3] = {h[0] / m1, h[1] / m1, h[2] / m1}, c1c1 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2];
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) J[a][b] -= m1 * ((a == b ? c1c1 : 0) - c1[a] * c1[b]);
    const double d1 = J[0][0], d2 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const double d3 = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                      J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
    if (!(d1 > 0 && d2 > 0 && d3 > 0))
        return fail(QG_ERR_ARG, "%s: %s: the FRAME's rotational inertia about its centre of mass is not positive definite with payload %g kg at (%g, %g, %g)",
                    who, what, dm, p[0], p[1], p[2]);
    return QG_OK;
}
// identity rows into the dynamics buffer (with them the per-env kernels compute the shared model's bits)
static int dyn_fill_identity(qg_sim *s, const char *who) {
    const size_t n = (size_t)s->n;
    float id[QG_NDYN];
    dyn_identity_row(s, id);
    float *h = (float *)malloc(n * QG_NDYN * sizeof(float));
    if (!h) return fail(QG_ERR_ALLOC, "out of host memory");
    for (int c = 0; c < QG_NDYN; c++)
        for (size_t i = 0; i < n; i++) h[c * n + i] = id[c];
    hipError_t e = hipMemcpy(s->d_dyn, h, n * QG_NDYN * sizeof(float), hipMemcpyHostToDevice);
    free(h);
    if (e != hipSuccess) return fail(QG_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return QG_OK;
}
// what the per-env kernels read behind the model tables: the dynamics rows' address, the wrench rows' address (NULL while wrench mode
// is off: the kernels' wave-uniform branch), the FRAME's centre of mass and the push schedule.  Callers have waited for the device.
static int model_dyn_upload(qg_sim *s) {
    KModelDyn h;
    h.rows = s->d_dyn;
    h.xfrc = s->xfrc ? s->d_xfrc : nullptr;
    for (int i = 0; i < 3; i++) h.com0[i] = (float)s->model.body_ipos[0][i];
    h.push = s->xfrc ? s->push : KPush{};
    const size_t off = offsetof(KModelDyn, rows);
    HIP_TRY(hipMemcpy((char *)s->d_model_dyn + off, (const char *)&h + off, sizeof(KModelDyn) - off, hipMemcpyHostToDevice), QG_ERR_DEVICE);
    return QG_OK;
}
// The per-env forms of the table-driven kernels, for per-env dynamics and for wrench mode alike: the dynamics rows (identity) and the
// kernels' model pointer.  Called when neither mode is on yet; `what` names the mode in the refusals.
static int per_env_enable(qg_sim *s, const char *who, const char *what) {
    if (s->mapping == QG_MAP_LANE || s->mapping == QG_MAP_PAIR)
        return fail(QG_ERR_ARG, "%s: %s run in the LINK and QUAD mappings only (qg_set_mapping AUTO, LINK or QUAD first)", who, what);
    if (s->res.active) return fail(QG_ERR_ARG, "%s: the resident step mode is on (qg_resident_stop first)", who);
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }   // steps of the shared model may be in flight on a caller's stream
    const size_t n = (size_t)s->n;
    if (!s->d_dyn && s->mem.alloc(s->d_dyn, n * QG_NDYN * sizeof(float))) return QG_ERR_ALLOC;
    if (!s->d_model_dyn && s->mem.alloc(s->d_model_dyn, sizeof(KModelDyn))) return QG_ERR_ALLOC;
    HIP_TRY(hipMemcpy(&s->d_model_dyn->m, s->d_model, sizeof(KModel), hipMemcpyDeviceToDevice), QG_ERR_DEVICE);
    int rc = dyn_fill_identity(s, who);
    if (rc != QG_OK) return rc;
    rc = model_dyn_upload(s);
    if (rc != QG_OK) return rc;
    s->baked = 0;
    return QG_OK;
}
// switch the mode on: the row buffer (identity rows) and the per-env kernels' model pointer, the table-driven kernels
static int dyn_enable(qg_sim *s, const char *who) {
    if (s->dyn) return QG_OK;
    if (!s->xfrc) {                 // (wrench mode runs the per-env kernels already, with identity rows)
        int rc = per_env_enable(s, who, "per-env dynamics");
        if (rc != QG_OK) return rc;
    }
    s->dyn = 1;
    return QG_OK;
}

extern "C" int qg_set_dynamics_range(qg_sim *s, const qg_dynamics_range *r) {
    if (!s || !r) return fail(QG_ERR_ARG, "qg_set_dynamics_range: null argument");
    for (int c = 0; c < QG_NDYN; c++)
        if (!(r->lo[c] <= r->hi[c])) return fail(QG_ERR_ARG, "qg_set_dynamics_range: column %d: lo %g > hi %g (or not a number)", c, (double)r->lo[c], (double)r->hi[c]);
    // every corner of (payload mass, x, y, z) and both ends of the other columns
    for (int corner = 0; corner < 16; corner++) {
        float row[QG_NDYN];
        for (int c = 0; c < QG_NDYN; c++) row[c] = r->lo[c];
        for (int b = 0; b < 4; b++) row[QG_DYN_PAYLOAD_MASS + b] = (corner >> b) & 1 ? r->hi[QG_DYN_PAYLOAD_MASS + b] : r->lo[QG_DYN_PAYLOAD_MASS + b];
        int rc = dyn_check_row(s, row, "qg_set_dynamics_range", "lo corner");
        if (rc != QG_OK) return rc;
        for (int c = 0; c < QG_NDYN; c++)
            if (c < QG_DYN_PAYLOAD_MASS || c > QG_DYN_PAYLOAD_Z) row[c] = r->hi[c];
        rc = dyn_check_row(s, row, "qg_set_dynamics_range", "hi corner");
        if (rc != QG_OK) return rc;
    }
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    int rc = dyn_enable(s, "qg_set_dynamics_range");
    if (rc != QG_OK) return rc;
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);        // (the range takes effect from the next call that draws)
    memcpy(s->dyn_range.lo, r->lo, sizeof r->lo);
    memcpy(s->dyn_range.hi, r->hi, sizeof r->hi);
    s->dyn_range_set = 1;
    return QG_OK;
}

extern "C" int qg_get_dynamics(qg_sim *s, float *rows) {
    if (!s || !rows) return fail(QG_ERR_ARG, "qg_get_dynamics: null argument");
    const size_t n = (size_t)s->n;
    if (!s->dyn) {
        float id[QG_NDYN];
        dyn_identity_row(s, id);
        for (size_t i = 0; i < n; i++) memcpy(rows + i * QG_NDYN, id, sizeof id);
        return QG_OK;
    }
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }
    float *h = (float *)malloc(n * QG_NDYN * sizeof(float));
    if (!h) return fail(QG_ERR_ALLOC, "out of host memory");
    hipError_t e = hipMemcpy(h, s->d_dyn, n * QG_NDYN * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        for (int c = 0; c < QG_NDYN; c++)
            for (size_t i = 0; i < n; i++) rows[i * QG_NDYN + c] = h[c * n + i];
    free(h);
    if (e != hipSuccess) return fail(QG_ERR_DEVICE, "qg_get_dynamics: %s", hipGetErrorString(e));
    return QG_OK;
}

extern "C" int qg_set_dynamics(qg_sim *s, const uint8_t *mask, const float *rows) {
    if (!s || !rows) return fail(QG_ERR_ARG, "qg_set_dynamics: null argument");
    const size_t n = (size_t)s->n;
    char what[48];
    for (size_t i = 0; i < n; i++) {
        if (mask && !mask[i]) continue;
        snprintf(what, sizeof what, "env %zu", i);
        int rc = dyn_check_row(s, rows + i * QG_NDYN, "qg_set_dynamics", what);
        if (rc != QG_OK) return rc;
    }
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    int rc = dyn_enable(s, "qg_set_dynamics");
    if (rc != QG_OK) return rc;
    // read-modify-write of the rows: steps (and their auto-reset draws) may be in flight on a caller's stream even when the mode was
    // already on (dyn_enable then returns at once) -- the header's ordering contract
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }
    float *h = (float *)malloc(n * QG_NDYN * sizeof(float));
    if (!h) return fail(QG_ERR_ALLOC, "out of host memory");
    hipError_t e = hipMemcpy(h, s->d_dyn, n * QG_NDYN * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) {
        for (size_t i = 0; i < n; i++)
            if (!mask || mask[i])
                for (int c = 0; c < QG_NDYN; c++) h[c * n + i] = rows[i * QG_NDYN + c];
        e = hipMemcpy(s->d_dyn, h, n * QG_NDYN * sizeof(float), hipMemcpyHostToDevice);
    }
    free(h);
    if (e != hipSuccess) return fail(QG_ERR_DEVICE, "qg_set_dynamics: %s", hipGetErrorString(e));
    return QG_OK;
}

extern "C" int qg_clear_dynamics(qg_sim *s) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if (!s->dyn) return QG_OK;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);        // per-env steps may be in flight on a caller's stream
    if (s->xfrc) {                  // wrench mode keeps the per-env kernels: identity rows
        int rc = dyn_fill_identity(s, "qg_clear_dynamics");
        if (rc != QG_OK) return rc;
    }
    s->dyn = 0;
    s->dyn_range_set = 0;
    if (!s->xfrc) s->baked = s->model_baked;
    return QG_OK;
}

// ------------------------------------------------------------------------------------------------------
// external wrenches and the push schedule (include/quadgym.h, QG_NXFRC columns per body)
// ------------------------------------------------------------------------------------------------------
static size_t xfrc_bytes(const qg_sim *s) { return (size_t)s->n * QG_NBODY * QG_NXFRC * sizeof(float); }
// switch wrench mode on: zero rows, no schedule, the per-env kernels (with identity dynamics rows unless that mode is on)
static int xfrc_enable(qg_sim *s, const char *who) {
    if (s->xfrc) return QG_OK;
    if (!s->dyn) {
        int rc = per_env_enable(s, who, "external wrenches");
        if (rc != QG_OK) return rc;
    } else {
        int rr = qg_retire_and_sync(s);        // per-env steps may be in flight on a caller's stream
        if (rr != QG_OK) return rr;
    }
    if (!s->d_xfrc && s->mem.alloc(s->d_xfrc, xfrc_bytes(s))) return QG_ERR_ALLOC;
    HIP_TRY(hipMemset(s->d_xfrc, 0, xfrc_bytes(s)), QG_ERR_DEVICE);
    s->push = KPush{};
    s->xfrc = 1;
    int rc = model_dyn_upload(s);
    if (rc != QG_OK) { s->xfrc = 0; return rc; }
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_set_xfrc(qg_sim *s, const uint8_t *mask, const float *rows) {
    if (!s || !rows) return fail(QG_ERR_ARG, "qg_set_xfrc: null argument");
    const size_t n = (size_t)s->n, w = QG_NBODY * QG_NXFRC;
    for (size_t i = 0; i < n; i++) {
        if (mask && !mask[i]) continue;
        for (size_t c = 0; c < w; c++) {     // (exponent bits: the device pass, which parses this too, assumes finite math)
            uint32_t bits;
            memcpy(&bits, rows + i * w + c, 4);
            if (((bits >> 23) & 0xFFu) == 0xFFu)
                return fail(QG_ERR_ARG, "qg_set_xfrc: env %zu, body %zu, column %zu is not finite", i, c / QG_NXFRC, c % QG_NXFRC);
        }
    }
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    int rc = xfrc_enable(s, "qg_set_xfrc");
    if (rc != QG_OK) return rc;
    // steps may be in flight on a caller's stream even when the mode was already on -- the header's ordering contract
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }
    if (!mask) {
        HIP_TRY(hipMemcpy(s->d_xfrc, rows, xfrc_bytes(s), hipMemcpyHostToDevice), QG_ERR_DEVICE);
        return QG_OK;
    }
    float *h = (float *)malloc(xfrc_bytes(s));
    if (!h) return fail(QG_ERR_ALLOC, "out of host memory");
    hipError_t e = hipMemcpy(h, s->d_xfrc, xfrc_bytes(s), hipMemcpyDeviceToHost);
    if (e == hipSuccess) {
        for (size_t i = 0; i < n; i++)
            if (mask[i]) memcpy(h + i * w, rows + i * w, w * sizeof(float));
        e = hipMemcpy(s->d_xfrc, h, xfrc_bytes(s), hipMemcpyHostToDevice);
    }
    free(h);
    if (e != hipSuccess) return fail(QG_ERR_DEVICE, "qg_set_xfrc: %s", hipGetErrorString(e));
    return QG_OK;
}

extern "C" int qg_set_xfrc_device(qg_sim *s, const float *d_rows, void *stream) {
    if (!s || !d_rows) return fail(QG_ERR_ARG, "qg_set_xfrc_device: null argument");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    if (!s->xfrc) {                 // the first call switches the mode on, which waits for the device (not while a stream is captured)
        int rc = xfrc_enable(s, "qg_set_xfrc_device");
        if (rc != QG_OK) return rc;
    }
    if (s->res.launched) {          // (the resident kernel cannot run in wrench mode; a stale launch is retired as launch_step does)
        int rr = resident_retire(s);
        if (rr != QG_OK) return rr;
    }
    const hipStream_t st = (hipStream_t)stream;
    note_caller_stream(s, st);
    HIP_TRY(hipMemcpyAsync(s->d_xfrc, d_rows, xfrc_bytes(s), hipMemcpyDeviceToDevice, st), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_get_xfrc(qg_sim *s, float *rows) {
    if (!s || !rows) return fail(QG_ERR_ARG, "qg_get_xfrc: null argument");
    if (!s->xfrc) {
        memset(rows, 0, xfrc_bytes(s));
        return QG_OK;
    }
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }
    HIP_TRY(hipMemcpy(rows, s->d_xfrc, xfrc_bytes(s), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    return QG_OK;
}

extern "C" int qg_set_push(qg_sim *s, const qg_push_params *p) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if (!p) {                       // the schedule off; the rows (and the mode) stay
        if (!s->xfrc) return QG_OK;
        HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
        { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }
        s->push = KPush{};
        return model_dyn_upload(s);
    }
    if (p->interval < 1) return fail(QG_ERR_ARG, "qg_set_push: interval %d < 1 env-step", p->interval);
    if (p->duration < 1 || p->duration > p->interval)
        return fail(QG_ERR_ARG, "qg_set_push: duration %d outside 1 .. interval (%d)", p->duration, p->interval);
    if (!(p->probability >= 0.f && p->probability <= 1.f)) return fail(QG_ERR_ARG, "qg_set_push: probability %g outside [0, 1]", (double)p->probability);
    uint32_t fmax_bits;
    memcpy(&fmax_bits, &p->force_max, 4);     // (exponent bits, as for the rows: the device pass assumes finite math)
    if (!(p->force_min >= 0.f && p->force_min <= p->force_max) || ((fmax_bits >> 23) & 0xFFu) == 0xFFu)
        return fail(QG_ERR_ARG, "qg_set_push: force range [%g, %g] (need 0 <= force_min <= force_max, finite)", (double)p->force_min, (double)p->force_max);
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    int rc = xfrc_enable(s, "qg_set_push");
    if (rc != QG_OK) return rc;
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }
    s->push.interval = p->interval;
    s->push.duration = p->duration;
    s->push.probability = p->probability;
    s->push.force_min = p->force_min;
    s->push.force_max = p->force_max;
    return model_dyn_upload(s);
}

extern "C" int qg_clear_xfrc(qg_sim *s) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if (!s->xfrc) return QG_OK;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    { int rr = qg_retire_and_sync(s); if (rr != QG_OK) return rr; }      // steps in wrench mode may be in flight on a caller's stream
    HIP_TRY(hipMemset(s->d_xfrc, 0, xfrc_bytes(s)), QG_ERR_DEVICE);
    s->xfrc = 0;
    s->push = KPush{};
    int rc = model_dyn_upload(s);
    if (rc != QG_OK) return rc;
    if (!s->dyn) s->baked = s->model_baked;
    return QG_OK;
}
