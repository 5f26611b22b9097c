// qg_po.hip -- the partially observable observation pack: its stand-alone kernels and the host side
// (qg_po_*); the per-env arithmetic and the row output live in qg_po_dev.h, which the fused step kernel shares.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>
#include <cstring>

#include "qg_sim.h"          // qg_sim, qg_walk; through it qg_po_dev.h

// Runs after the physics (and walking-reward) kernels of the step when the step kernel in use has no fused form of it.  A block of
// QG_PO_THREADS threads owns QG_PO_ENVS envs:
//   phase 1  one thread per env: orientation filter, the new 26-value frame and (for an env the step has just auto-reset) the
//            reset frame, into LDS (po_frame_env);
//   phase 2  all threads, 16 per env: the env's row of `out`, the new frame into the env's ring slot (po_emit_rows).
__global__ __launch_bounds__(QG_PO_THREADS) void qg_po_frame_kernel(KPoParams P, KPoState S, int n, const float *__restrict__ obs33,
                                   const float *__restrict__ eff_actions, const float *__restrict__ qpos /* [19][n] */,
                                   KWalkParams WP, KWalkState WS /* the commands live here */, const uint8_t *__restrict__ done,
                                   float *__restrict__ out /* [n][window*26] */, float *__restrict__ term_out /* [n][window*26] or NULL */,
                                   int sample_cmd, uint64_t seed, uint64_t env_index_base, const int32_t *__restrict__ episode) {
    __shared__ float s_new[QG_PO_ENVS][QG_PO_FRAME];     // the frame of this step
    __shared__ float s_rst[QG_PO_ENVS][QG_PO_FRAME];     // the frame reset() would return (only for envs that finished)
    __shared__ int s_slot[QG_PO_ENVS];                   // ring slot of the newest frame
    __shared__ int s_fin[QG_PO_ENVS];                    // the env finished and was auto-reset by the physics kernel
    const int env0 = blockIdx.x * QG_PO_ENVS;
    if (threadIdx.x < QG_PO_ENVS && env0 + threadIdx.x < n) {
        const int le = threadIdx.x, env = env0 + le;
        const PoEnvIn in = po_env_load(S, n, env);
        float *fr = s_new[le];
        for (int j = 0; j < 12; ++j) fr[11 + j] = fminf(fmaxf(eff_actions[(size_t)env * 12 + j], -1.f), 1.f);
        int slot, fin;
        po_frame_env(P, S, n, env, in, obs33 + (size_t)env * 33, qpos[3 * n + env], qpos[4 * n + env], qpos[5 * n + env], qpos[6 * n + env],
                     WS.vel[env], WS.vel[n + env], WS.head[env], WS.head[n + env], done[env] != 0, fr, s_rst[le], slot, fin);
        s_slot[le] = slot;
        s_fin[le] = fin;
        // random_controls on the device: the new episode's command, drawn only now that both frames show the old one
        if (fin && sample_cmd) walk_sample_command(WP, WS, n, env, seed, env_index_base, episode[env] - 1);
    }
    __syncthreads();
    po_emit_rows(P, S, n, env0, threadIdx.x >> 4, threadIdx.x & 15, s_new, s_rst, s_slot, s_fin, out, term_out);
}

// explicit (masked) reset: the stack is filled with the reset frame, the estimate aliases data.qpos[3:7] from now on
__global__ void qg_po_reset_kernel(KPoParams P, KPoState S, int n, const uint8_t *mask, const float *__restrict__ vel,
                                   const float *__restrict__ head, float *__restrict__ out /* nullable */) {
    const int env = blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= n) return;
    if (mask && !mask[env]) return;
    float q[4] = {S.orient[env], S.orient[n + env], S.orient[2 * n + env], S.orient[3 * n + env]};
    if (S.alias[env]) { q[0] = 1.f; q[1] = q[2] = q[3] = 0.f; }
    float roll, pitch, yaw;
    po_euler(q[0], q[1], q[2], q[3], roll, pitch, yaw);
    float rf[QG_PO_FRAME];
    for (int i = 0; i < 6; ++i) rf[i] = 0.f;
    rf[6] = roll; rf[7] = pitch; rf[8] = yaw; rf[9] = 0.f; rf[10] = 0.f;
    for (int j = 0; j < 12; ++j) rf[11 + j] = P.default_ctrl[j];
    rf[23] = vel[env]; rf[24] = vel[n + env]; rf[25] = po_atan2(head[n + env], head[env]);
    float *st = S.stack + 2 * (size_t)env * P.window * QG_PO_FRAME;       // the ring holds every frame twice (KPoState.stack)
    for (int f = 0; f < P.window; ++f)
        for (int i = 0; i < QG_PO_FRAME; ++i) {
            st[f * QG_PO_FRAME + i] = rf[i];
            st[(P.window + f) * QG_PO_FRAME + i] = rf[i];
            if (out) out[(size_t)env * P.window * QG_PO_FRAME + f * QG_PO_FRAME + i] = rf[i];
        }
    S.alias[env] = 1;
    S.nstep[env] = 0;
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
#define QG_BLOB_PO 0x4f505751u     /* "QWPO" */

struct qg_po {
    qg_walk *walk;
    KPoParams kp;
    KPoState st;
    QgDevMem mem;
    float *d_obs33, *d_out, *d_term;
};

extern "C" int qg_po_destroy(qg_po *p) {
    if (p) qg_free_handle(p, p->walk->sim->device);   // steps that read or write the frame ring may still be in flight on a caller's stream
    return QG_OK;
}

extern "C" int qg_po_obs_dim(const qg_po *p) { return p ? p->kp.window * QG_PO_FRAME : fail(QG_ERR_ARG, "null handle"); }

static int po_reset_kernel(qg_po *p, const uint8_t *dmask, float *d_out) {
    qg_sim *s = p->walk->sim;
    int threads = 256, blocks = (s->n + threads - 1) / threads;
    hipLaunchKernelGGL(qg_po_reset_kernel, dim3(blocks), dim3(threads), 0, s->stream, p->kp, p->st, s->n, dmask, (const float *)p->walk->st.vel,
                       (const float *)p->walk->st.head, d_out);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    HIP_TRY(hipStreamSynchronize(s->stream), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_po_create(qg_walk *w, int32_t obs_window, qg_po **out) {
    if (!w || !out) return fail(QG_ERR_ARG, "qg_po_create: null argument");
    *out = nullptr;
    if (obs_window < 1 || obs_window > 64) return fail(QG_ERR_ARG, "qg_po_create: obs_window must be in 1..64");
    qg_sim *s = w->sim;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    qg_po *p = qg_new_handle<qg_po>();
    if (!p) return QG_ERR_ALLOC;
    p->walk = w;
    KPoParams &k = p->kp;
    k.dt = (float)(s->model.timestep * s->task.frame_skip);          // po_walking_quad.py:18
    k.gain = 0.033f;                                                  // the library's default IMU gain
    // data.time > settling_time / 2 (:37): first substep count whose f64-accumulated clock exceeds it
    {
        double t = 0, half = w->params.settling_time / 2;
        int64_t c = 0;
        while (!(t > half) && c < INT32_MAX) { t += s->model.timestep; c++; }
        k.half_settle_substeps = (int32_t)c;
    }
    k.window = obs_window;
    k.frame_skip = s->task.frame_skip;
    k.auto_reset = s->task.auto_reset;
    for (int i = 0; i < QG_NU; i++) k.default_ctrl[i] = (float)s->task.default_ctrl[i];
    size_t n = (size_t)s->n, width = (size_t)obs_window * QG_PO_FRAME;
    // the ring keeps every frame twice (KPoState.stack); QG_PO_RING_SLACK bytes behind it: the fused forms' unpredicated 16-byte loads may
    // read that far past the last env's row (sized and asserted against the copy's batch shape next to QG_PO_COPY_K)
    QgDevMem &M = p->mem;
    if (M.alloc(p->st.orient, 4 * n * 4) || M.alloc(p->st.alias, n, true) || M.alloc(p->st.nstep, n * 4, true) ||
        M.alloc(p->st.stack, 2 * n * width * 4 + QG_PO_RING_SLACK, true) || M.alloc(p->st.head, n * 4, true) ||
        M.alloc(p->d_obs33, n * QG_NSENSOR * 4) || M.alloc(p->d_out, n * width * 4) || M.alloc(p->d_term, n * width * 4)) {
        qg_po_destroy(p);
        return QG_ERR_ALLOC;
    }
    QgHostBuf<float> h(4 * n);                                       // computed_orientation = [1, 0, 0, 0] (:19)
    if (h.oom()) {
        qg_po_destroy(p);
        return QG_ERR_ALLOC;
    }
    for (size_t i = 0; i < n; i++) { h[i] = 1.f; h[n + i] = h[2 * n + i] = h[3 * n + i] = 0.f; }
    const hipError_t e = hipMemcpy(p->st.orient, h, 4 * n * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        qg_po_destroy(p);
        return fail(QG_ERR_ALLOC, "qg_po_create: %s", hipGetErrorString(e));
    }
    *out = p;
    return QG_OK;
}

extern "C" int qg_po_reset(qg_po *p, const uint8_t *mask, uint64_t seed, uint32_t flags, float *obs) {
    if (!p) return fail(QG_ERR_ARG, "null handle");
    qg_sim *s = p->walk->sim;
    // refused before anything is launched: a refused call leaves the observation pack as it was
    if ((flags & QG_RESET_DYNAMICS) && !s->dyn_range_set) return fail(QG_ERR_ARG, "qg_po_reset: QG_RESET_DYNAMICS without a range (qg_set_dynamics_range)");
    // the reset frame shows the estimate and the command as they stand BEFORE the robots / commands are reset (:59-69)
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);   // device-pointer steps may be in flight on a caller's stream
    if (mask) HIP_TRY(hipMemcpy(s->d_mask, mask, (size_t)s->n, hipMemcpyHostToDevice), QG_ERR_DEVICE);
    QG_TRY(po_reset_kernel(p, mask ? s->d_mask : nullptr, p->d_out));
    if (obs) HIP_TRY(hipMemcpy(obs, p->d_out, (size_t)s->n * p->kp.window * QG_PO_FRAME * 4, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    return qg_walk_reset(p->walk, mask, seed, flags);
}

extern "C" int qg_po_step_device(qg_po *p, const float *actions, float *obs, float *reward, uint8_t *done, float *components,
                                 float *terminal_obs, void *stream) {
    if (!p || !actions || !obs || !reward || !done) return fail(QG_ERR_ARG, "qg_po_step_device: null argument");
    qg_walk *w = p->walk;
    qg_sim *s = w->sim;
    // up to 4096 envs the whole step -- physics, walking task layer, observation pack -- is ONE launch
    // (QG_PO_UNFUSED=1 at qg_create keeps the separate observation-pack launch: the A/B and the parity test of the two forms)
    if (qg_walk_fused(s) && qg_po_fusable(s) && !s->po_unfused) {
        KPoLaunch pl;
        pl.P = p->kp;
        pl.S = p->st;
        pl.out = obs;
        pl.term_out = terminal_obs;
        pl.sample = w->kp.cmd_sample ? 1 : 0;
        return qg_walk_step_core(w, actions, nullptr, reward, done, components, stream, true, &pl);
    }
    QG_TRY(qg_walk_step_core(w, actions, p->d_obs33, reward, done, components, stream, true));
    int blocks = (s->n + QG_PO_ENVS - 1) / QG_PO_ENVS;
    hipLaunchKernelGGL(qg_po_frame_kernel, dim3(blocks), dim3(QG_PO_THREADS), 0, (hipStream_t)stream, p->kp, p->st, s->n, (const float *)p->d_obs33,
                       (const float *)w->st.eff_actions, (const float *)s->st.qpos, w->kp, w->st, (const uint8_t *)done, obs, terminal_obs,
                       w->kp.cmd_sample ? 1 : 0, s->seed, s->env_index_base, (const int32_t *)s->st.episode);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_po_step(qg_po *p, const float *actions, float *obs, float *reward, uint8_t *done, float *components, float *terminal_obs) {
    if (!p || !actions || !obs || !reward || !done) return fail(QG_ERR_ARG, "qg_po_step: null argument");
    qg_walk *w = p->walk;
    qg_sim *s = w->sim;
    const size_t n = (size_t)s->n, width = (size_t)p->kp.window * QG_PO_FRAME;
    const HostOut out[4] = {{obs, p->d_out, n * width * 4}, {reward, w->d_reward, n * 4}, {done, w->d_done, n},
                            {components, w->d_comps, n * QG_NWALKREWARD * 4}};
    QG_TRY(host_step(s, actions, w->d_actions, out, [&] {
        return qg_po_step_device(p, w->d_actions, p->d_out, w->d_reward, w->d_done, components ? w->d_comps : nullptr,
                                 terminal_obs ? p->d_term : nullptr, s->stream);
    }));
    if (terminal_obs) {
        // the terminal stacks only exist for envs that finished: the [n][obs_dim] transfer (4.3 MB at 4096 envs and window 10 -- as much
        // as the observation itself) is skipped on the steps where none did
        bool any = false;
        for (size_t i = 0; i < n && !any; i++) any = done[i] != 0;
        if (any) HIP_TRY(hipMemcpy(terminal_obs, p->d_term, n * width * 4, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    }
    return QG_OK;
}

static int po_fields(const qg_po *p, QgField *f) {
    const size_t n = (size_t)p->walk->sim->n, width = (size_t)p->kp.window * QG_PO_FRAME;
    const QgField all[] = {{p->st.orient, 4 * n * 4}, {p->st.alias, n}, {p->st.nstep, n * 4}, {p->st.stack, 2 * n * width * 4}, {p->st.head, n * 4}};
    const int k = (int)(sizeof all / sizeof all[0]);
    if (f) memcpy(f, all, sizeof all);
    return k;
}
extern "C" int64_t qg_po_state_bytes(const qg_po *p) {
    if (!p) return fail(QG_ERR_ARG, "null handle");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_bytes(f, po_fields(p, f));
}
extern "C" int qg_po_get_state(qg_po *p, void *blob) {
    if (!p || !blob) return fail(QG_ERR_ARG, "qg_po_get_state: null argument");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_out(p->walk->sim, QG_BLOB_PO, p->kp.window, f, po_fields(p, f), blob);
}
extern "C" int qg_po_set_state(qg_po *p, const void *blob) {
    if (!p || !blob) return fail(QG_ERR_ARG, "qg_po_set_state: null argument");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_in(p->walk->sim, QG_BLOB_PO, p->kp.window, f, po_fields(p, f), blob, "qg_po_set_state");
}
