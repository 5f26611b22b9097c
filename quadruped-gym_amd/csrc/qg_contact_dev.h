// qg_contact_dev.h -- the device code of foot-contact sensing (include/quadgym.h: qg_contact_*) and the qg_contact handle,
// shared by the kernels that evaluate it: qg_contact_kernel (qg_contact.hip, the sensor's read), qg_gait_kernel (qg_gait.hip, the same
// read with the gait-shaped reward terms reduced behind it in the same launch) and qg_priv_kernel (qg_priv.hip, the forces and foot
// heights of the privileged state pack).  Internal: not installed, nothing in here is
// exported.  Same text, same arithmetic, same rounding in every kernel: the gait launch reports the sensor's bits.
//
// Layout of a wave.  The work is latency-bound (about 150 B in and 350 B out per env), so the launch is shaped like the headline
// step's: one body per lane, 16 lanes per env (13 working, 3 idle), 4 envs per wave -- 4096 envs are 1024 waves, one per SIMD.  Every
// lane walks its own chain from the FRAME (at most three links) and carries pose and velocity with it: the arithmetic is redundant
// between the lanes of a leg, but there is no LDS, no barrier and no cross-lane hand-off.  The lane then runs its body's 8 or 12
// sample points; the four foot lanes also advance their foot's timers and write its 48-byte row with three 16-byte stores.
//
// No atomics; no lane reads what another lane of the launch writes, with one exception inside a wave: the four foot lanes of an env
// read its `armed` word and foot 0's lane then sets it -- one wave, the load ahead of the store in program order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qg_sim.h"          // qg_sim (its state arrays, model tables and dynamics rows), qg_blob_*

#define QGC_ENVS 16          // envs per 256-thread workgroup: 16 lanes each
#define QGC_NFOOT 4

struct KContact {
    int32_t n, advance;
    int32_t done_kind, done_stride;
    float threshold, dt;
};

struct qg_contact {
    qg_sim *sim;
    qg_contact_desc desc;
    QgDevMem mem;
    int4 *d_timers;           // [n][4]
    int32_t *d_armed;         // [n]
    float *d_force, *d_feet;  // staging of qg_contact_read
};

// the launch constants of a read of `c` as the simulator stands at this call (qg_set_task may change frame_skip)
static inline KContact qgc_args(const qg_contact *c, const void *done, int32_t done_kind, int32_t done_stride, int32_t advance) {
    KContact A;
    A.n = c->sim->n, A.advance = advance ? 1 : 0;
    A.done_kind = done_kind, A.done_stride = done ? done_stride : 1;
    A.threshold = c->desc.force_threshold;
    A.dt = (float)(c->sim->model.timestep * c->sim->task.frame_skip);
    return A;
}

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

// R0 = R(qpos[3:7] / |qpos[3:7]|) of env e, row-major: the FRAME's orientation (also what the privileged state pack rotates with)
__device__ __forceinline__ void qgc_frame_rot(const float *__restrict__ sq /* [19][n] */, size_t n, size_t e, float *R) {
    float qw = qgc_at(sq, 3, n, e), qx = qgc_at(sq, 4, n, e), qy = qgc_at(sq, 5, n, e), qz = qgc_at(sq, 6, n, e);
    const float inv = 1.0f / sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
    qw *= inv, qx *= inv, qy *= inv, qz *= inv;
    R[0] = 1.f - 2.f * (qy * qy + qz * qz); R[1] = 2.f * (qx * qy - qw * qz);       R[2] = 2.f * (qx * qz + qw * qy);
    R[3] = 2.f * (qx * qy + qw * qz);       R[4] = 1.f - 2.f * (qx * qx + qz * qz); R[5] = 2.f * (qy * qz - qw * qx);
    R[6] = 2.f * (qx * qz - qw * qy);       R[7] = 2.f * (qy * qz + qw * qx);       R[8] = 1.f - 2.f * (qx * qx + qy * qy);
}

// Body b (0 .. QG_NBODY - 1) of env e: the world position x and velocity v of its frame origin and the ground reaction force F on it.
// DYN: friction and the contact stiffness / damping scales come from the env's dynamics row ([QG_NDYN][n]).  Reads only; crosses no lane.
template <bool DYN>
__device__ __forceinline__ void qgc_body(const KModel *__restrict__ M, const float *__restrict__ sq /* [19][n] */, const float *__restrict__ sv /* [18][n] */,
                                         const float *__restrict__ dyn, int b, size_t e, size_t n, float *x, float *v, float *F) {
    // ---- the FRAME ------------------------------------------------------------------------------------------------------------------
    float R[9], w[3];
    {
        qgc_frame_rot(sq, n, e, R);
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
    F[0] = active ? -ct * vP[0] : 0.f, F[1] = active ? -ct * vP[1] : 0.f, F[2] = active ? Fn : 0.f;
}

// A foot lane (foot f = 0..3 of env e): the foot's timers as this sample leaves them (t: prev_contact, phase_steps, last_air_steps,
// last_stance_steps) and its events.  With A.advance the update rule of include/quadgym.h is applied and written back.
__device__ __forceinline__ void qgc_foot_timers(const KContact &A, const void *done, int4 *timers /* [n][4] */, int32_t *armed /* [n] */, size_t e, int f,
                                                int contact, int4 &t, int &touchdown, int &liftoff) {
    const size_t foot = e * QGC_NFOOT + (size_t)f;
    t = timers[foot];
    touchdown = 0, liftoff = 0;
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
        if (f == 0) armed[e] = 1;                             // (behind every foot lane's load of it: one wave, program order)
    }
}

// ... and its row of `feet` (QG_FOOT_*): three 16-byte stores
__device__ __forceinline__ void qgc_foot_row(float *feet, size_t e, int f, const float *x, const float *v, int contact, int touchdown, int liftoff, int4 t,
                                             float dt) {
    float4 *o = reinterpret_cast<float4 *>(feet + (e * QGC_NFOOT + (size_t)f) * QG_FOOT_DIM);
    o[0] = make_float4(x[0], x[1], x[2], v[0]);
    o[1] = make_float4(v[1], v[2], (float)contact, (float)touchdown);
    o[2] = make_float4((float)liftoff, (float)t.y * dt, (float)t.z * dt, (float)t.w * dt);
}
