// qg_sim_multi.hip -- the simulator's host side of many env-steps per launch: the sequence forms (qg_step_device_seq) and the
// resident form of the one-link-per-lane kernel (qg_resident_*: mailbox, launch, retire, rings and their reports).  No device code:
// the kernels and their launchers are the step-kernel units' (qg_step_launch.h; qg_kernel_resident.hip).
#include <cstring>

#include "qg_step_launch.h"

int qg_multi_step_usable(const qg_sim *s, const char *who) {
    if (qg_effective_mapping(s) != QG_MAP_LINK)
        return fail(QG_ERR_ARG, "%s: needs the one-link-per-lane mapping (AUTO up to 4096 envs, lagged sensors)", who);
    if (s->n > s->simds * QGK_LINK_ENVS) return fail(QG_ERR_ARG, "%s: at most %d envs (one wave per SIMD)", who, s->simds * QGK_LINK_ENVS);
    if (s->walk_bound) return fail(QG_ERR_ARG, "%s: a walking task layer is bound to this handle", who);
    if (qg_jitter_at_reset(s))
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
    QG_TRY(qg_refuse_per_env(s, "qg_step_device_seq: not available with %s (%s first)"));
    if (s->walk_bound) return fail(QG_ERR_ARG, "qg_step_device_seq: a walking task layer is bound to this handle");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    if (s->res.launched) QG_TRY(qg_resident_retire(s));
    hipStream_t st = (hipStream_t)stream;
    const int emap = qg_effective_mapping(s);
    // the two-legs-per-lane mapping (16 385 .. 32 768 envs, >= 57 344) and the one-leg-per-lane mapping on the grids AUTO gives it
    // (four-wave workgroups) have one-launch forms of their own
    const bool seq_pair = emap == QG_MAP_PAIR && qg_sim_baked(s) && s->task.sensor_lag && !qg_jitter_at_reset(s);
    const bool seq_quad = emap == QG_MAP_QUAD && s->task.sensor_lag && quad_wg4(s) && !qg_jitter_at_reset(s);
    if (!seq_pair && !seq_quad && qg_multi_step_usable(s, "qg_step_device_seq") != QG_OK) {
        // another mapping (more than one wave per SIMD of the one-link-per-lane kernel), or hinge jitter behind every step: the same
        // rows from `count` per-step launches -- the call means the same thing for every handle, the one-launch form is the fast path
        const size_t arow = (size_t)s->n * QG_NU, prow = (size_t)s->n * (s->obs_dim + 2);
        for (int32_t k = 0; k < count; k++)
            QG_TRY(qg_launch_step(s, actions + k * arow, nullptr, nullptr, nullptr, nullptr, packed + k * prow, st));
        return QG_OK;
    }
    qg_note_caller_stream(s, st);
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

void qg_resident_free(qg_sim *s) {
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
int qg_resident_retire(qg_sim *s) {
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
    QG_TRY(qg_multi_step_usable(s, "resident kernel launch"));
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
    QG_TRY(qg_refuse_per_env(s, "qg_resident_start: not available with %s (%s first)"));
    if (slots < 1 || slots > 4096) return fail(QG_ERR_ARG, "qg_resident_start: slots must be 1..4096");
    if (idle_timeout_us == 0) idle_timeout_us = 2000;
    if (idle_timeout_us < 50 || idle_timeout_us > 100000) return fail(QG_ERR_ARG, "qg_resident_start: idle_timeout_us must be 50..100000 (0 = 2000)");
    QG_TRY(qg_multi_step_usable(s, "qg_resident_start"));
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
        qg_resident_free(s);
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
    QG_TRY(qg_retire_and_sync(s));
    qg_resident_free(s);
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
        QG_TRY(qg_resident_retire(s));
    }
    return resident_launch(s);        // stream-ordered behind the launch that has left (or is leaving)
}

extern "C" int qg_resident_step_device(qg_sim *s, int32_t count, void *stream) {
    if (!s || count < 1) return fail(QG_ERR_ARG, "qg_resident_step_device: bad argument");
    if (!s->res.active) return fail(QG_ERR_ARG, "qg_resident_step_device: the resident step mode is off (qg_resident_start)");
    if (count > s->res.k.slots) return fail(QG_ERR_ARG, "qg_resident_step_device: count %d exceeds the %d slots of the mailbox", count, s->res.k.slots);
    if ((hipStream_t)stream == s->stream) return fail(QG_ERR_ARG, "qg_resident_step_device: that is the stream the resident kernel occupies");
    QG_TRY(resident_check_reports(s, "qg_resident_step_device"));
    QG_TRY(qg_resident_ensure(s));
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
