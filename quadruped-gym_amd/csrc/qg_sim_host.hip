// qg_sim_host.hip -- the simulator's host-pointer path: the page-locked arena of a handle, and the entry points that take and return
// ordinary host memory through it -- qg_step, qg_step_mirror, qg_get_state, qg_set_state -- with the two halves of host_step (qg_sim.h)
// that the task layers' host-pointer steps share.  No device code: the step is qg_launch_step's, the transposes are the core's
// (qg_capi.hip).
#include <cstring>

#include "qg_sim.h"

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
    QG_TRY(qg_resident_retire(s));
    if (!s->caller_inflight && !s->captured_once) return QG_OK;
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    s->caller_inflight = 0;
    return QG_OK;
}

static int copy_in(qg_sim *s, const float *host, float *field_major, int w) {
    if (!host) return QG_OK;
    HIP_TRY(hipMemcpyAsync(s->d_stage, host, (size_t)s->n * w * sizeof(float), hipMemcpyHostToDevice, s->stream), QG_ERR_DEVICE);
    QG_TRY(qg_transpose_in_launch(s, s->d_stage, field_major, w));
    HIP_TRY(hipStreamSynchronize(s->stream), QG_ERR_LAUNCH);
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
    for (int f = 0; f < 4; f++) {
        float *stage = s->d_stage + soff;
        soff += n * w[f];
        if (!so[f].user) continue;
        QG_TRY(qg_transpose_out_launch(s, src[f], stage, w[f]));
        QG_TRY(pin_out_enqueue(s, so[f], stage));
    }
    return pin_out_enqueue(s, so[4], s->st.nstep);
}

extern "C" int qg_get_state(qg_sim *s, float *qpos, float *qvel, float *act, float *ctrl, int32_t *nstep) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    QG_TRY(qg_retire_and_sync(s));   // steps may be in flight on a caller's stream
    // every transfer enqueued, ONE synchronisation (five synchronised round trips made the single-env facade's mirror of the state
    // 120 us of a 160 us step)
    PinOut so[5];
    QG_TRY(pin_reserve(s, state_out_layout(s, {qpos, qvel, act, ctrl, nstep}, 0, so)));
    QG_TRY(state_out_enqueue(s, so));
    HIP_TRY(hipStreamSynchronize(s->stream), QG_ERR_LAUNCH);
    for (int f = 0; f < 5; f++) pin_out_finish(s, so[f]);
    return QG_OK;
}

// the two halves of host_step (qg_sim.h) around the step's own launch
int qg_host_step_begin(qg_sim *s, const float *actions, float *d_actions, const HostOut (&out)[4], const StateDst *state, HostStep &h) {
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    QG_TRY(wait_for_caller_streams(s));
    size_t off = pin_align((size_t)s->n * QG_NU * sizeof(float));
    for (int i = 0; i < 4; i++) { h.o[i] = {out[i].user, off, out[i].bytes}; off += pin_align(h.o[i].bytes); }
    if (state) off = state_out_layout(s, *state, off, h.state);
    QG_TRY(pin_reserve(s, off));
    return pin_actions_in(s, actions, d_actions);
}
int qg_host_step_end(qg_sim *s, const HostOut (&out)[4], const StateDst *state, const HostStep &h) {
    for (int i = 0; i < 4; i++) QG_TRY(pin_out_enqueue(s, h.o[i], out[i].dev));
    if (state) QG_TRY(state_out_enqueue(s, h.state));
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
    QG_TRY(qg_retire_and_sync(s));
    QG_TRY(copy_in(s, qpos, s->st.qpos, QG_NQ));
    QG_TRY(copy_in(s, qvel, s->st.qvel, QG_NV));
    QG_TRY(copy_in(s, act, s->st.act, QG_NU));
    QG_TRY(copy_in(s, ctrl, s->st.ctrl, QG_NU));
    if (nstep) HIP_TRY(hipMemcpy(s->st.nstep, nstep, (size_t)s->n * sizeof(int32_t), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    return QG_OK;
}
