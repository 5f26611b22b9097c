// qg_contact.hip -- foot-contact sensing on the state a simulator holds in device memory (include/quadgym.h: qg_contact_*, DESIGN
// 4.15): the ground reaction force of every body, the feet's position and velocity, contact flags and integer gait timers.  ONE
// launch, which only reads the simulator's arrays and model tables; it shares no device code with the step kernels.
//
// Layout of a wave.  The work is latency-bound (about 150 B in and 350 B out per env), so the launch is shaped like the headline
// step's: one body per lane, 16 lanes per env (13 working, 3 idle), 4 envs per wave -- 4096 envs are 1024 waves, one per SIMD.  Every
// lane walks its own chain from the FRAME (at most three links) and carries pose and velocity with it: the arithmetic is redundant
// between the lanes of a leg, but there is no LDS, no barrier and no cross-lane hand-off.  The lane then runs its body's 8 or 12
// sample points; the four foot lanes also advance their foot's timers and write its 48-byte row with three 16-byte stores.
//
// No atomics; no lane reads what another lane of the launch writes, with one exception inside a wave: the four foot lanes of an env
// read its `armed` word and foot 0's lane then sets it -- one wave, the load ahead of the store in program order.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <new>

#include "qg_sim.h"          // qg_sim (its state arrays, model tables and dynamics rows), qg_blob_*

#define QGC_ENVS 16          // envs per 256-thread workgroup: 16 lanes each
#define QGC_NFOOT 4

struct KContact {
    int32_t n, advance;
    int32_t done_kind, done_stride;
    float threshold, dt;
};

// field-major state ([width][n]): row r of env e
__device__ __forceinline__ float qgc_at(const float *__restrict__ a, int r, size_t n, size_t e) { return a[(size_t)r * n + e]; }

// out = M v (M row-major)
__device__ __forceinline__ void qgc_rot(const float *M, const float *v, float *out) {
    out[0] = M[0] * v[0] + M[1] * v[1] + M[2] * v[2];
    out[1] = M[3] * v[0] + M[4] * v[1] + M[5] * v[2];
    out[2] = M[6] * v[0] + M[7] * v[1] + M[8] * v[2];
}
// out = a x b
__device__ __forceinline__ void qgc_cross(const float *a, const float *b, float *out) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// DYN: friction and the contact stiffness / damping scales come from the env's dynamics row ([QG_NDYN][n])
template <bool DYN>
__global__ __launch_bounds__(QGC_ENVS * 16) void qg_contact_kernel(KContact A, const KModel *__restrict__ M, const float *__restrict__ sq /* [19][n] */,
                                                                   const float *__restrict__ sv /* [18][n] */, const float *__restrict__ dyn,
                                                                   const void *done, int4 *timers /* [n][4] */, int32_t *armed /* [n] */,
                                                                   float *__restrict__ body_force, float *__restrict__ feet) {
    const int b = threadIdx.x & 15;
    const int64_t e64 = (int64_t)blockIdx.x * QGC_ENVS + (threadIdx.x >> 4);
    if (e64 >= A.n || b >= QG_NBODY) return;              // the tail and the three idle lanes: nothing below crosses lanes
    const size_t e = (size_t)e64, n = (size_t)A.n;

    // ---- the FRAME ------------------------------------------------------------------------------------------------------------------
    float x[3], R[9], v[3], w[3];
    {
        float qw = qgc_at(sq, 3, n, e), qx = qgc_at(sq, 4, n, e), qy = qgc_at(sq, 5, n, e), qz = qgc_at(sq, 6, n, e);
        const float inv = 1.0f / sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
        qw *= inv, qx *= inv, qy *= inv, qz *= inv;
        R[0] = 1.f - 2.f * (qy * qy + qz * qz); R[1] = 2.f * (qx * qy - qw * qz);       R[2] = 2.f * (qx * qz + qw * qy);
        R[3] = 2.f * (qx * qy + qw * qz);       R[4] = 1.f - 2.f * (qx * qx + qz * qz); R[5] = 2.f * (qy * qz - qw * qx);
        R[6] = 2.f * (qx * qz - qw * qy);       R[7] = 2.f * (qy * qz + qw * qx);       R[8] = 1.f - 2.f * (qx * qx + qy * qy);
        const float wl[3] = {qgc_at(sv, 3, n, e), qgc_at(sv, 4, n, e), qgc_at(sv, 5, n, e)};
        qgc_rot(R, wl, w);
        for (int d = 0; d < 3; ++d) x[d] = qgc_at(sq, d, n, e), v[d] = qgc_at(sv, d, n, e);
    }

    // ---- this lane's chain: links j0 .. j0 + links - 1 of its leg -------------------------------------------------------------------------
    const int links = b ? (b - 1) % 3 + 1 : 0, j0 = b ? (b - 1) / 3 * 3 : 0;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        if (s < links) {
            const KLink &L = M->link[j0 + s];
            const float ang = qgc_at(sq, 7 + j0 + s, n, e) - L.ref, qd = qgc_at(sv, 6 + j0 + s, n, e);
            float off[3], lin[3], Am[9], sn, cs;
            qgc_rot(R, L.pos, off);                           // x_b - x_p
            qgc_cross(w, off, lin);
            for (int d = 0; d < 3; ++d) x[d] += off[d], v[d] += lin[d];
            for (int r = 0; r < 3; ++r)                          // R_p Q_b
                for (int c = 0; c < 3; ++c) Am[3 * r + c] = R[3 * r] * L.Q[c] + R[3 * r + 1] * L.Q[3 + c] + R[3 * r + 2] * L.Q[6 + c];
            sincosf(ang, &sn, &cs);
            for (int r = 0; r < 3; ++r) {                        // ... Rz(ang)
                R[3 * r] = cs * Am[3 * r] + sn * Am[3 * r + 1];
                R[3 * r + 1] = cs * Am[3 * r + 1] - sn * Am[3 * r];
                R[3 * r + 2] = Am[3 * r + 2];
                w[r] += R[3 * r + 2] * qd;
            }
        }
    }

    // ---- the body's sample points ----------------------------------------------------------------------------------------------------
    const float(*cp)[3] = b ? M->link[b - 1].cp : M->cp0;
    const int ncp = b ? QGK_CP_LINK : QGK_CP_FRAME;
    const float margin = M->contact_margin;
    float S = 0.f, sr[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < QGK_CP_FRAME; ++i) {
        if (i < ncp) {
            float r[3];
            qgc_rot(R, cp[i], r);
            const float pen = margin - (x[2] + r[2]);
            if (pen > 0.f) {
                S += pen;
                for (int d = 0; d < 3; ++d) sr[d] += pen * r[d];
            }
        }
    }

    // ---- the contact law ----------------------------------------------------------------------------------------------------------------
    float kc = M->contact_k, cmax = M->contact_c, mu = M->contact_mu;
    if constexpr (DYN) {
        mu = qgc_at(dyn, QG_DYN_FRICTION, n, e);
        kc *= qgc_at(dyn, QG_DYN_CONTACT_STIFFNESS_SCALE, n, e);
        cmax *= qgc_at(dyn, QG_DYN_CONTACT_DAMPING_SCALE, n, e);
    }
    const bool active = S > 0.f;
    const float inv = 1.0f / (active ? S : 1.0f);
    const float P[3] = {sr[0] * inv, sr[1] * inv, sr[2] * inv};   // centre of pressure about the body origin
    float vP[3];
    qgc_cross(w, P, vP);
    for (int d = 0; d < 3; ++d) vP[d] += v[d];
    const float W = kc * S, c = cmax * fminf(S * M->contact_inv_ramp, 1.0f);
    const float Fn = fmaxf(W - c * vP[2], 0.f);
    const float speed = sqrtf(vP[0] * vP[0] + vP[1] * vP[1]);
    const bool sliding = c * speed > mu * Fn;
    const float ct = sliding ? mu * Fn / speed : c;
    const float F[3] = {active ? -ct * vP[0] : 0.f, active ? -ct * vP[1] : 0.f, active ? Fn : 0.f};
    if (body_force) {
        float *o = body_force + (e * QG_NBODY + (size_t)b) * 3;
        o[0] = F[0], o[1] = F[1], o[2] = F[2];
    }

    // ---- the feet: timers and rows ------------------------------------------------------------------------------------------------------
    if (links != 3) return;
    const size_t foot = e * QGC_NFOOT + (size_t)(j0 / 3);
    const int contact = F[2] > A.threshold ? 1 : 0;
    int4 t = timers[foot];                                    // prev_contact, phase_steps, last_air_steps, last_stance_steps
    int touchdown = 0, liftoff = 0;
    if (A.advance) {
        bool fresh = armed[e] == 0;
        if (done) fresh |= qg_done_at(done, A.done_kind, A.done_stride, e);
        if (fresh) {
            t.y = 1, t.z = 0, t.w = 0;
        } else if (contact == t.x) {
            t.y += 1;
        } else {
            if (contact) t.z = t.y, touchdown = 1;
            else t.w = t.y, liftoff = 1;
            t.y = 1;
        }
        t.x = contact;
        timers[foot] = t;
        if (j0 == 0) armed[e] = 1;                           // (behind every foot lane's load of it: one wave, program order)
    }
    if (feet) {
        float4 *o = reinterpret_cast<float4 *>(feet + foot * QG_FOOT_DIM);
        o[0] = make_float4(x[0], x[1], x[2], v[0]);
        o[1] = make_float4(v[1], v[2], (float)contact, (float)touchdown);
        o[2] = make_float4((float)liftoff, (float)t.y * A.dt, (float)t.z * A.dt, (float)t.w * A.dt);
    }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
#define QG_BLOB_CONTACT 0x54435751u     /* "QWCT" */

struct qg_contact {
    qg_sim *sim;
    qg_contact_desc desc;
    QgDevMem mem;
    int4 *d_timers;           // [n][4]
    int32_t *d_armed;         // [n]
    float *d_force, *d_feet;  // staging of qg_contact_read
};

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
        int32_t *h = new (std::nothrow) int32_t[n];
        if (!h) return fail(QG_ERR_ALLOC, "out of host memory");
        hipError_t e = hipMemcpy(h, c->d_armed, n * sizeof(int32_t), hipMemcpyDeviceToHost);
        for (size_t i = 0; i < n && e == hipSuccess; i++)
            if (mask[i]) h[i] = 0;
        if (e == hipSuccess) e = hipMemcpy(c->d_armed, h, n * sizeof(int32_t), hipMemcpyHostToDevice);
        delete[] h;
        if (e != hipSuccess) return fail(QG_ERR_DEVICE, "qg_contact_reset: %s", hipGetErrorString(e));
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
    KContact A;
    A.n = s->n, A.advance = advance ? 1 : 0;
    A.done_kind = done_kind, A.done_stride = done ? done_stride : 1;
    A.threshold = c->desc.force_threshold;
    A.dt = (float)(s->model.timestep * s->task.frame_skip);       // the task as it stands at this call (qg_set_task may change frame_skip)
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
    if ((uintptr_t)feet & 15) return fail(QG_ERR_ARG, "qg_contact_read_device: feet must be 16-byte aligned");
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
