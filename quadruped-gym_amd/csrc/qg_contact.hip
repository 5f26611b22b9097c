// qg_contact.hip -- foot-contact sensing on the state a simulator holds in device memory (include/quadgym.h: qg_contact_*, DESIGN
// 4.15): the ground reaction force of every body, the feet's position and velocity, contact flags and integer gait timers.  ONE
// launch, which only reads the simulator's arrays and model tables; it shares no device code with the step kernels.  The device code
// of a lane and the layout of a wave are in qg_contact_dev.h, which the gait-reward launch (qg_gait.hip) shares.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "qg_contact_dev.h"

template <bool DYN>
__global__ __launch_bounds__(QGC_ENVS * 16) void qg_contact_kernel(KContact A, const KModel *__restrict__ M, const float *__restrict__ sq /* [19][n] */,
                                                                   const float *__restrict__ sv /* [18][n] */, const float *__restrict__ dyn,
                                                                   const void *done, int4 *timers /* [n][4] */, int32_t *armed /* [n] */,
                                                                   float *__restrict__ body_force, float *__restrict__ feet) {
    const int b = threadIdx.x & 15;
    const int64_t e64 = (int64_t)blockIdx.x * QGC_ENVS + (threadIdx.x >> 4);
    if (e64 >= A.n || b >= QG_NBODY) return;              // the tail and the three idle lanes: nothing below crosses lanes
    const size_t e = (size_t)e64, n = (size_t)A.n;

    float x[3], v[3], F[3];
    qgc_body<DYN>(M, sq, sv, dyn, b, e, n, x, v, F);
    if (body_force) {
        float *o = body_force + (e * QG_NBODY + (size_t)b) * 3;
        o[0] = F[0], o[1] = F[1], o[2] = F[2];
    }

    // ---- the feet: timers and rows ------------------------------------------------------------------------------------------------------
    if (b == 0 || (b - 1) % 3 != 2) return;
    const int f = (b - 1) / 3;
    const int contact = F[2] > A.threshold ? 1 : 0;
    int4 t;
    int touchdown, liftoff;
    qgc_foot_timers(A, done, timers, armed, e, f, contact, t, touchdown, liftoff);
    if (feet) qgc_foot_row(feet, e, f, x, v, contact, touchdown, liftoff, t, A.dt);
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
#define QG_BLOB_CONTACT 0x54435751u     /* "QWCT" */

extern "C" int qg_contact_destroy(qg_contact *c) {
    if (c) qg_free_handle(c, c->sim->device);      // reads may still be in flight on a caller's stream
    return QG_OK;
}

extern "C" int qg_contact_create(qg_sim *s, const qg_contact_desc *desc, qg_contact **out) {
    if (!out) return fail(QG_ERR_ARG, "qg_contact_create: null output");
    *out = nullptr;
    if (!desc) return fail(QG_ERR_ARG, "qg_contact_create: null description");
    QG_CHECK_STRUCT(desc, qg_contact_desc);
    if (desc->reserved != 0) return fail(QG_ERR_ARG, "qg_contact: reserved must be 0");
    if (!qg_finite32(desc->force_threshold) || desc->force_threshold < 0.f)
        return fail(QG_ERR_ARG, "qg_contact: force_threshold %g must be finite and >= 0", desc->force_threshold);
    if (!s) return fail(QG_ERR_ARG, "qg_contact_create: null simulator");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    qg_contact *c = qg_new_handle<qg_contact>();
    if (!c) return QG_ERR_ALLOC;
    c->sim = s;
    c->desc = *desc;
    const size_t n = (size_t)s->n;
    if (c->mem.alloc(c->d_timers, n * QGC_NFOOT * sizeof(int4), true) || c->mem.alloc(c->d_armed, n * sizeof(int32_t), true) ||
        c->mem.alloc(c->d_force, n * QG_CONTACT_FORCE_DIM * sizeof(float)) || c->mem.alloc(c->d_feet, n * QG_CONTACT_FEET_DIM * sizeof(float))) {
        qg_contact_destroy(c);
        return QG_ERR_ALLOC;
    }
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        qg_contact_destroy(c);
        return fail(QG_ERR_DEVICE, "qg_contact_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return QG_OK;
}

extern "C" int qg_contact_reset(qg_contact *c, const uint8_t *mask) {
    if (!c) return fail(QG_ERR_ARG, "qg_contact_reset: null handle");
    const size_t n = (size_t)c->sim->n;
    HIP_TRY(hipSetDevice(c->sim->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);           // a read may be in flight on a caller's stream
    if (!mask) {
        HIP_TRY(hipMemset(c->d_armed, 0, n * sizeof(int32_t)), QG_ERR_DEVICE);
    } else {
        QgHostBuf<int32_t> h(n);
        QG_TRY(h.oom());
        HIP_TRY(hipMemcpy(h, c->d_armed, n * sizeof(int32_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
        for (size_t i = 0; i < n; i++)
            if (mask[i]) h[i] = 0;
        HIP_TRY(hipMemcpy(c->d_armed, h, n * sizeof(int32_t), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    }
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);
    return QG_OK;
}

// everything a read can be refused for, before anything is launched
static int contact_check(const qg_contact *c, const void *done, int32_t done_kind, int32_t done_stride, const float *body_force, const float *feet,
                         const char *who) {
    if (!body_force && !feet) return fail(QG_ERR_ARG, "%s: body_force and feet are both NULL", who);
    if (!c) return fail(QG_ERR_ARG, "%s: null handle", who);
    QG_TRY(qg_check_done(who, done, done_kind, done_stride));
    if (c->sim->res.active) return fail(QG_ERR_ARG, "%s: the resident step mode is on, the state lives in registers (qg_resident_stop first)", who);
    return QG_OK;
}

static int contact_launch(qg_contact *c, const void *done, int32_t done_kind, int32_t done_stride, int32_t advance, float *body_force, float *feet,
                          hipStream_t stream) {
    qg_sim *s = c->sim;
    const KContact A = qgc_args(c, done, done_kind, done_stride, advance);     // the task as it stands at this call
    const dim3 grid((unsigned)((s->n + QGC_ENVS - 1) / QGC_ENVS)), block(QGC_ENVS * 16);
    if (s->dyn)
        hipLaunchKernelGGL(qg_contact_kernel<true>, grid, block, 0, stream, A, (const KModel *)s->d_model, (const float *)s->st.qpos,
                           (const float *)s->st.qvel, (const float *)s->d_dyn, done, c->d_timers, c->d_armed, body_force, feet);
    else
        hipLaunchKernelGGL(qg_contact_kernel<false>, grid, block, 0, stream, A, (const KModel *)s->d_model, (const float *)s->st.qpos,
                           (const float *)s->st.qvel, (const float *)nullptr, done, c->d_timers, c->d_armed, body_force, feet);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_contact_read_device(qg_contact *c, const void *done, int32_t done_kind, int32_t done_stride, int32_t advance, float *body_force,
                                      float *feet, void *stream) {
    QG_TRY(contact_check(c, done, done_kind, done_stride, body_force, feet, "qg_contact_read_device"));
    if (!qg_aligned(feet, 16)) return fail(QG_ERR_ARG, "qg_contact_read_device: feet must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->sim->device), QG_ERR_DEVICE);
    qg_note_caller_stream(c->sim, (hipStream_t)stream);          // a later host-pointer call of the simulator waits for this read
    return contact_launch(c, done, done_kind, done_stride, advance, body_force, feet, (hipStream_t)stream);
}

extern "C" int qg_contact_read(qg_contact *c, float *body_force, float *feet) {
    QG_TRY(contact_check(c, nullptr, 0, 0, body_force, feet, "qg_contact_read"));
    qg_sim *s = c->sim;
    const size_t n = (size_t)s->n;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);           // steps may be in flight on a caller's stream
    QG_TRY(contact_launch(c, nullptr, 0, 0, 0, body_force ? c->d_force : nullptr, feet ? c->d_feet : nullptr, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream), QG_ERR_LAUNCH);
    if (body_force) HIP_TRY(hipMemcpy(body_force, c->d_force, n * QG_CONTACT_FORCE_DIM * sizeof(float), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    if (feet) HIP_TRY(hipMemcpy(feet, c->d_feet, n * QG_CONTACT_FEET_DIM * sizeof(float), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    return QG_OK;
}

static int contact_fields(const qg_contact *c, QgField *f) {
    const size_t n = (size_t)c->sim->n;
    const QgField all[] = {{c->d_timers, n * QGC_NFOOT * sizeof(int4)}, {c->d_armed, n * sizeof(int32_t)}};
    const int k = (int)(sizeof all / sizeof all[0]);
    if (f) memcpy(f, all, sizeof all);
    return k;
}
extern "C" int64_t qg_contact_state_bytes(const qg_contact *c) {
    if (!c) return fail(QG_ERR_ARG, "null handle");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_bytes(f, contact_fields(c, f));
}
extern "C" int qg_contact_get_state(qg_contact *c, void *blob) {
    if (!c || !blob) return fail(QG_ERR_ARG, "qg_contact_get_state: null argument");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_out(c->sim, QG_BLOB_CONTACT, 0, f, contact_fields(c, f), blob);
}
extern "C" int qg_contact_set_state(qg_contact *c, const void *blob) {
    if (!c || !blob) return fail(QG_ERR_ARG, "qg_contact_set_state: null argument");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_in(c->sim, QG_BLOB_CONTACT, 0, f, contact_fields(c, f), blob, "qg_contact_set_state");
}
