// qg_priv.hip -- the privileged state pack (include/quadgym.h: qg_priv_*): ONE launch that writes, per env, the joint row
// [ actor observation | QG_PRIV_DIM columns of the simulator's truth ] an asymmetric critic reads.  It only reads the simulator's
// arrays and model tables.  The ground forces, the feet's height and the threshold comparison are the contact sensor's device code
// (qg_contact_dev.h: qgc_body), the FRAME's wrench with the scheduled push is the step kernels' (qg_step_dev.h: xfrc_frame, push_force):
// the columns are those launches' bits.
//
// A wave is laid out as the sensor's: one body per lane, 16 lanes per env (13 bodies, 3 idle), 4 envs per wave.  As in qg_gait.hip all
// 16 lanes of a live env stay in one control flow (the idle lanes repeat body 12's arithmetic on valid addresses and store none of
// it); only a whole 16-lane group past n leaves, together.  What the 16 lanes store:
//   cols 0-8     lanes 0..8, one each: each forms R0 with the sensor's function (qgc_frame_rot) and keeps its column
//   cols 9-45    the 37 copy-through columns of qpos / qvel / act: lane l takes 9 + l, 25 + l, 41 + l -- a group's stores of a round are
//                16 consecutive floats
//   cols 46-65   the four foot lanes (3, 6, 9, 12): flag, force xyz, height of their foot
//   col 66       the count of the env's non-foot flags in the wave's ballot (exact; the count qg_gait.hip reduces), lane 15
//   cols 67-84   dynamics row, FRAME wrench, episode time: lane l takes 67 + l, lanes 0 and 1 also 83 and 84
//   obs          the 16 lanes copy the row in front, 16 bytes per lane and round under the alignment rule of qg_norm.hip, else 4
// No LDS, no barrier, no atomics; no lane reads what another lane of the launch writes (obs and out may not overlap).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qg_step_dev.h"         // xfrc_frame / push_force: the wrench the next env-step applies to the FRAME
#include "qg_contact_dev.h"      // qgc_body: the sensor's forces and body positions

struct KPriv {
    float threshold, timestep, friction;      // friction: column 0 of the identity dynamics row
    int32_t obs_stride, obs_dim, out_stride, vec;
};

// value `k` of (a0, a1, ...): a select chain over scalars, so that nothing is indexed by a lane-dependent number (an indexed private
// array would be placed in LDS or scratch)
__device__ __forceinline__ float qgp_pick3(int k, float a0, float a1, float a2) { return k == 2 ? a2 : k == 1 ? a1 : a0; }
__device__ __forceinline__ float qgp_pick6(int k, float a0, float a1, float a2, float a3, float a4, float a5) {
    return k >= 3 ? qgp_pick3(k - 3, a3, a4, a5) : qgp_pick3(k, a0, a1, a2);
}

template <bool DYN>
__global__ __launch_bounds__(QGC_ENVS * 16) void qg_priv_kernel(KPriv A, KStepArgs P, const KModel *__restrict__ M, const KTask *__restrict__ T,
                                                                const KModelDyn *__restrict__ Md /* NULL: wrench mode off */,
                                                                const float *__restrict__ dyn, const float *__restrict__ obs,
                                                                float *__restrict__ out) {
    const int lane = threadIdx.x & 15;
    const int64_t e64 = (int64_t)blockIdx.x * QGC_ENVS + (threadIdx.x >> 4);
    if (e64 >= P.n) return;                               // a whole 16-lane group: what is below crosses the lanes of a group only
    const size_t e = (size_t)e64, n = (size_t)P.n;
    const bool live = lane < QG_NBODY;
    const int b = live ? lane : QG_NBODY - 1;             // an idle lane stays in the control flow: body 12 again, nothing of it stored
    const float *sq = P.st.qpos, *sv = P.st.qvel;
    float *row = out + e * (size_t)A.out_stride + A.obs_dim;

    // ---- the observation in front ------------------------------------------------------------------------------------------------------
    if (A.obs_dim > 0) {
        const float *from = obs + e * (size_t)A.obs_stride;
        float *to = out + e * (size_t)A.out_stride;
        if (A.vec) {
            const float4 *f4 = reinterpret_cast<const float4 *>(from);
            float4 *t4 = reinterpret_cast<float4 *>(to);
            for (int c = lane; c < A.obs_dim / 4; c += 16) t4[c] = f4[c];
        } else {
            for (int c = lane; c < A.obs_dim; c += 16) to[c] = from[c];
        }
    }

    // ---- the sensor's part: forces, positions, flags ---------------------------------------------------------------------------------------
    float x[3], v[3], F[3];
    qgc_body<DYN>(M, sq, sv, dyn, b, e, n, x, v, F);
    const bool on_ground = live && F[2] > A.threshold;    // the foot flag's exact f32 comparison, for every body
    if (live && b != 0 && (b - 1) % 3 == 2) {
        const int f = (b - 1) / 3;
        row[QG_PRIV_FOOT_CONTACT + f] = on_ground ? 1.f : 0.f;
        float *o = row + QG_PRIV_FOOT_FORCE + 3 * f;
        o[0] = F[0], o[1] = F[1], o[2] = F[2];
        row[QG_PRIV_FOOT_HEIGHT + f] = x[2];
    }
    const unsigned group = (unsigned)(__ballot(on_ground) >> (threadIdx.x & 48)) & 0xffffu;     // the env's 16 flags
    const unsigned foot_lanes = (1u << 3) | (1u << 6) | (1u << 9) | (1u << 12);
    if (lane == 15) row[QG_PRIV_BODY_CONTACT] = (float)__popc(group & ~foot_lanes);

    // ---- the base: R0 as the sensor forms it --------------------------------------------------------------------------------------------------
    if (lane < 9) {
        float R[9];
        qgc_frame_rot(sq, n, e, R);
        const float vx = qgc_at(sv, 0, n, e), vy = qgc_at(sv, 1, n, e), vz = qgc_at(sv, 2, n, e);
        // R0^T v (the sums in the order of qgc_rot), qvel[3:6], -R0's third row; lane l keeps column l
        const float lin = qgp_pick3(lane, R[0] * vx + R[3] * vy + R[6] * vz, R[1] * vx + R[4] * vy + R[7] * vz, R[2] * vx + R[5] * vy + R[8] * vz);
        const float grav = qgp_pick3(lane - QG_PRIV_GRAVITY_DIR, -R[6], -R[7], -R[8]);
        row[lane] = lane < QG_PRIV_BASE_ANG_VEL ? lin : lane < QG_PRIV_GRAVITY_DIR ? qgc_at(sv, lane, n, e) : grav;
    }

    // ---- the copy-through columns 9 .. 45: qpos[2], qpos[7:19], qvel[6:18], act -------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int c = QG_PRIV_BASE_HEIGHT + 16 * k + lane;
        if (c < QG_PRIV_FOOT_CONTACT) {
            const float *src = c < QG_PRIV_JOINT_VEL ? sq : c < QG_PRIV_ACT ? sv : (const float *)P.st.act;
            const int r = c == QG_PRIV_BASE_HEIGHT ? 2 : c < QG_PRIV_JOINT_VEL ? c - QG_PRIV_JOINT_POS + 7 : c < QG_PRIV_ACT ? c - QG_PRIV_JOINT_VEL + 6
                                                                                                                             : c - QG_PRIV_ACT;
            row[c] = qgc_at(src, r, n, e);
        }
    }

    // ---- dynamics row, the FRAME's wrench of the next env-step, episode time: columns 67 .. 84 ---------------------------------------------
    KWrench w = {v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f)};
    if (Md) w = xfrc_frame(Md, P, (int)e, T->frame_skip);      // wave-uniform
    const float time = __fmul_rn((float)P.st.nstep[e], A.timestep);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = QG_PRIV_DYNAMICS + 16 * k + lane;
        if (c < QG_PRIV_DIM) {
            float val;
            if (c < QG_PRIV_FRAME_WRENCH) {
                const int d = c - QG_PRIV_DYNAMICS;
                if constexpr (DYN) val = qgc_at(dyn, d, n, e);
                else val = d == QG_DYN_FRICTION ? A.friction : d <= QG_DYN_PAYLOAD_Z ? 0.f : 1.f;
            } else {
                val = c == QG_PRIV_EPISODE_TIME ? time : qgp_pick6(c - QG_PRIV_FRAME_WRENCH, w.F.x, w.F.y, w.F.z, w.T.x, w.T.y, w.T.z);
            }
            row[c] = val;
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
struct qg_priv {
    qg_sim *sim;
    qg_priv_desc desc;
    QgDevMem mem;
    float *d_stage;           // [n][QG_PRIV_DIM]: staging of qg_priv_read
};

extern "C" int qg_priv_destroy(qg_priv *p) {
    if (p) qg_free_handle(p, p->sim->device);      // reads may still be in flight on a caller's stream
    return QG_OK;
}

extern "C" int qg_priv_create(qg_sim *s, const qg_priv_desc *desc, qg_priv **out) {
    if (!out) return fail(QG_ERR_ARG, "qg_priv_create: null output");
    *out = nullptr;
    if (!desc) return fail(QG_ERR_ARG, "qg_priv_create: null description");
    QG_CHECK_STRUCT(desc, qg_priv_desc);
    if (desc->reserved != 0) return fail(QG_ERR_ARG, "qg_priv: reserved must be 0");
    if (!qg_finite32(desc->force_threshold) || desc->force_threshold < 0.f)
        return fail(QG_ERR_ARG, "qg_priv: force_threshold %g must be finite and >= 0", desc->force_threshold);
    if (!s) return fail(QG_ERR_ARG, "qg_priv_create: null simulator");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    qg_priv *p = qg_new_handle<qg_priv>();
    if (!p) return QG_ERR_ALLOC;
    p->sim = s;
    p->desc = *desc;
    if (p->mem.alloc(p->d_stage, (size_t)s->n * QG_PRIV_DIM * sizeof(float))) {
        qg_priv_destroy(p);
        return QG_ERR_ALLOC;
    }
    *out = p;
    return QG_OK;
}

// everything a read can be refused for, before anything is launched
static int priv_check(const qg_priv *p, const float *obs, int32_t obs_stride, int32_t obs_dim, const float *out, int32_t out_stride, const char *who) {
    if (!out) return fail(QG_ERR_ARG, "%s: null output", who);
    if (obs_dim < 0) return fail(QG_ERR_ARG, "%s: obs_dim %d must be >= 0", who, obs_dim);
    if (!obs && obs_dim != 0) return fail(QG_ERR_ARG, "%s: obs_dim %d without obs", who, obs_dim);
    if (obs && obs_stride < obs_dim) return fail(QG_ERR_ARG, "%s: obs_stride %d must be >= obs_dim %d", who, obs_stride, obs_dim);
    if ((int64_t)out_stride < (int64_t)obs_dim + QG_PRIV_DIM)
        return fail(QG_ERR_ARG, "%s: out_stride %d must be >= obs_dim + %d = %lld", who, out_stride, QG_PRIV_DIM, (long long)obs_dim + QG_PRIV_DIM);
    if (!p) return fail(QG_ERR_ARG, "%s: null handle", who);
    if (obs && obs_dim > 0 && qg_rows_overlap(obs, obs_stride, obs_dim, out, out_stride, obs_dim + QG_PRIV_DIM, p->sim->n))
        return fail(QG_ERR_ARG, "%s: obs and out overlap", who);
    if (p->sim->res.active) return fail(QG_ERR_ARG, "%s: the resident step mode is on, the state lives in registers (qg_resident_stop first)", who);
    return QG_OK;
}

static int priv_launch(qg_priv *p, const float *obs, int32_t obs_stride, int32_t obs_dim, float *out, int32_t out_stride, hipStream_t stream) {
    qg_sim *s = p->sim;
    KPriv A;
    A.threshold = p->desc.force_threshold, A.timestep = (float)s->model.timestep, A.friction = (float)s->model.contact_friction;
    A.obs_stride = obs_stride, A.obs_dim = obs_dim, A.out_stride = out_stride;
    A.vec = (obs_dim > 0 && obs_dim % 4 == 0 && obs_stride % 4 == 0 && out_stride % 4 == 0 && qg_aligned(obs, 16) && qg_aligned(out, 16)) ? 1 : 0;
    KStepArgs P;                                           // what xfrc_frame reads of a step's arguments: the state and the random key
    memset(&P, 0, sizeof P);
    P.st = s->st, P.n = s->n, P.seed = s->seed, P.env_index_base = s->env_index_base;
    const KModelDyn *Md = s->xfrc ? s->d_model_dyn : nullptr;
    const dim3 grid((unsigned)((s->n + QGC_ENVS - 1) / QGC_ENVS)), block(QGC_ENVS * 16);
    if (s->dyn)
        hipLaunchKernelGGL(qg_priv_kernel<true>, grid, block, 0, stream, A, P, (const KModel *)s->d_model, (const KTask *)s->d_task, Md,
                           (const float *)s->d_dyn, obs, out);
    else
        hipLaunchKernelGGL(qg_priv_kernel<false>, grid, block, 0, stream, A, P, (const KModel *)s->d_model, (const KTask *)s->d_task, Md,
                           (const float *)nullptr, obs, out);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_priv_read_device(qg_priv *p, const float *obs, int32_t obs_stride, int32_t obs_dim, float *out, int32_t out_stride, void *stream) {
    QG_TRY(priv_check(p, obs, obs_stride, obs_dim, out, out_stride, "qg_priv_read_device"));
    HIP_TRY(hipSetDevice(p->sim->device), QG_ERR_DEVICE);
    qg_note_caller_stream(p->sim, (hipStream_t)stream);          // a later host-pointer call of the simulator waits for this read
    return priv_launch(p, obs, obs_stride, obs_dim, out, out_stride, (hipStream_t)stream);
}

extern "C" int qg_priv_read(qg_priv *p, float *host_out) {
    if (!p) return fail(QG_ERR_ARG, "qg_priv_read: null handle");
    if (!host_out) return fail(QG_ERR_ARG, "qg_priv_read: null output");
    qg_sim *s = p->sim;
    if (s->res.active) return fail(QG_ERR_ARG, "qg_priv_read: the resident step mode is on, the state lives in registers (qg_resident_stop first)");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);           // steps may be in flight on a caller's stream
    QG_TRY(priv_launch(p, nullptr, 0, 0, p->d_stage, QG_PRIV_DIM, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream), QG_ERR_LAUNCH);
    HIP_TRY(hipMemcpy(host_out, p->d_stage, (size_t)s->n * QG_PRIV_DIM * sizeof(float), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    return QG_OK;
}
