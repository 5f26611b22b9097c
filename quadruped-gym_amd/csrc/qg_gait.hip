// qg_gait.hip -- gait-shaped reward terms from the foot-contact sensor (include/quadgym.h: qg_gait_*): ONE launch that IS
// the sensor's read of its env-step (qg_contact_dev.h: forces, foot rows, timers, advance / done semantics, the same bits) and reduces
// the seven terms per env, weights them, sums them onto the reward and writes the component columns behind it.
//
// A wave is laid out as the sensor's: one body per lane, 16 lanes per env (13 working, 3 idle), 4 envs per wave.  Unlike the sensor's
// kernel this one crosses lanes, so all 16 lanes of a live env stay in one control flow up to the reduction: the idle lanes repeat body
// 12's arithmetic on valid addresses, store nothing and contribute exact zeros; only a whole 16-lane group past n leaves, together.
// The reduction: the feet's five float contributions are fetched from lanes 3, 6, 9, 12 of the group by 16-wide shuffles and added in
// ascending foot order by every lane; the contact flags are counted from the wave's ballot.  No LDS, no barrier, no atomics.  Every lane
// of the group then holds the env's seven components; lanes 0..6 store one each, lane 7 the reward, and the 16 lanes copy the base columns.
//
// No lane reads what another workgroup writes (reward in place: one lane loads and stores the element; base columns at the front of
// the same wide buffer: the copy is skipped); the `armed` word keeps the sensor's one-wave load-then-store order.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qg_contact_dev.h"
#include "qg_shaped_dev.h"

struct KGait {
    float w[QG_GAIT_NTERMS];
    float air_time_target, clearance_target, max_contact_force, min_command_speed;
    KShapedIO io;
};

template <bool DYN>
__global__ __launch_bounds__(QGC_ENVS * 16) void qg_gait_kernel(KContact A, KGait G, const KModel *__restrict__ M, const float *__restrict__ sq /* [19][n] */,
                                                                const float *__restrict__ sv /* [18][n] */, const float *__restrict__ dyn,
                                                                const void *done, int4 *timers /* [n][4] */, int32_t *armed /* [n] */,
                                                                float *body_force, float *feet, const float *reward, float *reward_out,
                                                                const float *base, float *comps, const float *command) {
    const int lane = threadIdx.x & 15;
    const int64_t e64 = (int64_t)blockIdx.x * QGC_ENVS + (threadIdx.x >> 4);
    if (e64 >= A.n) return;                               // a whole 16-lane group: what is below crosses the lanes of a group only
    const size_t e = (size_t)e64, n = (size_t)A.n;
    const bool live = lane < QG_NBODY;
    const int b = live ? lane : QG_NBODY - 1;             // an idle lane stays in the control flow: body 12 again, nothing stored

    float x[3], v[3], F[3];
    qgc_body<DYN>(M, sq, sv, dyn, b, e, n, x, v, F);
    if (live && body_force) {
        float *o = body_force + (e * QG_NBODY + (size_t)b) * 3;
        o[0] = F[0], o[1] = F[1], o[2] = F[2];
    }

    // ---- the feet: timers and rows, as the sensor's read; this lane's share of the five summed terms ---------------------------------------
    const bool on_ground = live && F[2] > A.threshold;     // the foot flag's exact f32 comparison, for every body
    float a_air = 0.f, a_slip = 0.f, a_clear = 0.f, a_down = 0.f, a_force = 0.f;
    if (live && b != 0 && (b - 1) % 3 == 2) {
        const int f = (b - 1) / 3, contact = on_ground ? 1 : 0;
        int4 t;
        int touchdown, liftoff;
        qgc_foot_timers(A, done, timers, armed, e, f, contact, t, touchdown, liftoff);
        if (feet) qgc_foot_row(feet, e, f, x, v, contact, touchdown, liftoff, t, A.dt);
        const float planar = v[0] * v[0] + v[1] * v[1], lift = x[2] - G.clearance_target;
        a_air = touchdown ? __fsub_rn(__fmul_rn((float)t.z, A.dt), G.air_time_target) : 0.f;     // the row's LAST_AIR_TIME, rounded as stored
        a_slip = contact ? planar : 0.f;
        a_clear = contact ? 0.f : lift * lift * sqrtf(planar);
        a_down = touchdown ? v[2] * v[2] : 0.f;
        a_force = fmaxf(F[2] - G.max_contact_force, 0.f);
    }

    // ---- the reduction over the 16 lanes of the env: every lane of the group is here ------------------------------------------------------
    float s_air, s_slip, s_clear, s_down, s_force;
    {
        s_air = __shfl(a_air, 3, 16), s_slip = __shfl(a_slip, 3, 16), s_clear = __shfl(a_clear, 3, 16);
        s_down = __shfl(a_down, 3, 16), s_force = __shfl(a_force, 3, 16);
#pragma unroll
        for (int src = 6; src <= 12; src += 3) {           // feet 1, 2, 3: ascending
            s_air = __fadd_rn(s_air, __shfl(a_air, src, 16)), s_slip = __fadd_rn(s_slip, __shfl(a_slip, src, 16));
            s_clear = __fadd_rn(s_clear, __shfl(a_clear, src, 16)), s_down = __fadd_rn(s_down, __shfl(a_down, src, 16));
            s_force = __fadd_rn(s_force, __shfl(a_force, src, 16));
        }
    }
    const unsigned group = (unsigned)(__ballot(on_ground) >> (threadIdx.x & 48)) & 0xffffu;     // the env's 16 flags
    const unsigned foot_lanes = (1u << 3) | (1u << 6) | (1u << 9) | (1u << 12);
    const int feet_down = __popc(group & foot_lanes), bodies_down = __popc(group & ~foot_lanes);

    // ---- the env's terms, weighted; every lane of the group holds them all ----------------------------------------------------------------
    bool moving = true;
    if (command) {
        const float *c = command + e * (size_t)G.io.command_stride;
        moving = QG_SHAPED_SPEED(c) > G.min_command_speed;
    }
    const bool finished = done ? qg_done_at(done, A.done_kind, A.done_stride, e) : false;
    const float term[QG_GAIT_NTERMS] = {moving ? s_air : 0.f, s_slip, s_clear, s_down, s_force, (float)bodies_down, feet_down == 0 ? 1.f : 0.f};
    // ---- the tail of a shaped-reward kernel (qg_shaped_dev.h): comp[], their sum, the component columns and the reward ----------------------
    QG_SHAPED_WEIGH(QG_GAIT_NTERMS, G.w, term, __fmul_rn, __fadd_rn)
    QG_SHAPED_STORE(QG_GAIT_NTERMS, G.io, __fadd_rn)
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
struct qg_gait {
    qg_contact *contact;
    qg_gait_desc desc;
    QgDevMem mem;             // empty: the handle has no device state of its own
};

extern "C" int qg_gait_destroy(qg_gait *g) {
    if (g) qg_free_handle(g, g->contact->sim->device);     // launches may still be in flight on a caller's stream
    return QG_OK;
}

extern "C" int qg_gait_create(qg_contact *contact, const qg_gait_desc *desc, qg_gait **out) {
    if (!out) return fail(QG_ERR_ARG, "qg_gait_create: null output");
    *out = nullptr;
    if (!desc) return fail(QG_ERR_ARG, "qg_gait_create: null description");
    QG_CHECK_STRUCT(desc, qg_gait_desc);
    if (desc->reserved != 0) return fail(QG_ERR_ARG, "qg_gait: reserved must be 0");
    QG_TRY(qg_check_weights(desc->weights, QG_GAIT_NTERMS, "qg_gait"));
    const struct { const char *name; float v; } lim[] = {{"air_time_target", desc->air_time_target}, {"clearance_target", desc->clearance_target},
                                                         {"max_contact_force", desc->max_contact_force}, {"min_command_speed", desc->min_command_speed}};
    for (const auto &l : lim)
        if (!qg_finite32(l.v) || l.v < 0.f) return fail(QG_ERR_ARG, "qg_gait: %s %g must be finite and >= 0", l.name, l.v);
    if (!contact) return fail(QG_ERR_ARG, "qg_gait_create: null contact sensor");
    qg_gait *g = qg_new_handle<qg_gait>();
    if (!g) return QG_ERR_ALLOC;
    g->contact = contact;
    g->desc = *desc;
    *out = g;
    return QG_OK;
}

extern "C" int qg_gait_set_weights(qg_gait *g, const float *weights) {
    if (!g || !weights) return fail(QG_ERR_ARG, "qg_gait_set_weights: null argument");
    QG_TRY(qg_check_weights(weights, QG_GAIT_NTERMS, "qg_gait_set_weights"));
    memcpy(g->desc.weights, weights, sizeof g->desc.weights);     // read by the next launch; a captured launch keeps its own copy
    return QG_OK;
}

extern "C" int qg_gait_reward_device(qg_gait *g, const void *done, int32_t done_kind, int32_t done_stride, int32_t advance, const float *reward,
                                   int32_t reward_stride, float *reward_out, int32_t reward_out_stride, float *components,
                                   int32_t components_stride, const float *base_components, int32_t base_stride, int32_t base_terms,
                                   const float *command, int32_t command_stride, float *body_force, float *feet, void *stream) {
    const char *who = "qg_gait_reward_device";
    if (!g) return fail(QG_ERR_ARG, "%s: null handle", who);
    if (!components && !reward_out) return fail(QG_ERR_ARG, "%s: components and reward_out are both NULL", who);
    QG_TRY(qg_check_done(who, done, done_kind, done_stride));
    qg_contact *c = g->contact;
    qg_sim *s = c->sim;
    KGait G;
    QG_TRY(qg_shaped_io(who, QG_GAIT_NTERMS, reward, reward_stride, reward_out, reward_out_stride, components, components_stride, base_components,
                        base_stride, base_terms, command, command_stride, s->n, &G.io));
    if (!qg_aligned(feet, 16)) return fail(QG_ERR_ARG, "%s: feet must be 16-byte aligned", who);
    if (s->res.active) return fail(QG_ERR_ARG, "%s: the resident step mode is on, the state lives in registers (qg_resident_stop first)", who);

    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    qg_note_caller_stream(s, (hipStream_t)stream);               // a later host-pointer call of the simulator waits for this launch
    const KContact A = qgc_args(c, done, done_kind, done_stride, advance);
    memcpy(G.w, g->desc.weights, sizeof G.w);
    G.air_time_target = g->desc.air_time_target, G.clearance_target = g->desc.clearance_target;
    G.max_contact_force = g->desc.max_contact_force, G.min_command_speed = g->desc.min_command_speed;
    const dim3 grid((unsigned)((s->n + QGC_ENVS - 1) / QGC_ENVS)), block(QGC_ENVS * 16);
    if (s->dyn)
        hipLaunchKernelGGL(qg_gait_kernel<true>, grid, block, 0, (hipStream_t)stream, A, G, (const KModel *)s->d_model, (const float *)s->st.qpos,
                           (const float *)s->st.qvel, (const float *)s->d_dyn, done, c->d_timers, c->d_armed, body_force, feet, reward, reward_out,
                           base_components, components, command);
    else
        hipLaunchKernelGGL(qg_gait_kernel<false>, grid, block, 0, (hipStream_t)stream, A, G, (const KModel *)s->d_model, (const float *)s->st.qpos,
                           (const float *)s->st.qvel, (const float *)nullptr, done, c->d_timers, c->d_armed, body_force, feet, reward, reward_out,
                           base_components, components, command);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}
