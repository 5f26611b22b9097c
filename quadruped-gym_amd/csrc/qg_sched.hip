// qg_sched.hip -- the commanded gait schedule (include/quadgym.h: qg_sched_*): ONE launch behind the env-step that advances
// every env's phase oscillator, compares the feet with the schedule in four reward terms -- forces, foot kinematics and contact flags
// by the sensor's own device code (qg_contact_dev.h: qgc_body), the sensor's timers and armed flags untouched --, adds the weighted
// terms onto the reward, writes the component columns and widens the observation row by the ten clock columns.
//
// A wave is laid out as the sensor's: one body per lane, 16 lanes per env (13 working, 3 idle), 4 envs per wave.  As in qg_gait.hip all
// 16 lanes of a live env stay in one control flow up to the reduction (the idle lanes repeat body 12's arithmetic on valid addresses,
// store nothing of it and contribute exact zeros); only a whole 16-lane group past n leaves, together.  What the lanes of a group do:
//   lane 0         the env's integer work: it alone loads phi and episode, hashes the key (three draws of the running episode, three more
//                  of the next one where the env finished), advances the phase and, last, stores the two words.  The (phase, gait row,
//                  frequency) of the row and of the terminal row go to the group by 16-wide shuffles.
//   lanes 3 6 9 12 their foot's s_f and hard_f and its share of the three summed terms, fetched by shuffles and added in ascending foot
//                  order by every lane; contact_match is counted from the wave's ballot.
//   lanes 0..9     one clock column each;  lanes 0..3 one component each, lane 4 the reward;  all 16 copy the base columns and the
//                  observation row (260 floats at obs_window = 10: 16 bytes per lane and round where alignment allows).
// No LDS, no barrier, no atomics.  No lane reads what another workgroup writes (a row in place is not copied at all; reward in place:
// one lane loads and stores the element).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qg_contact_dev.h"
#include "qg_key_dev.h"
#include "qg_shaped_dev.h"

#define QGS_SALT 0x5147534348454431ull                            // "QGSCHED1"
#define QGS_ROW 5                                                 // u32 per row of the table in device memory: off_f[4], D
#define QGS_BLOB 0x48435351u                                      /* "QSCH" */
#define QGS_MUL(a, b) ((a) * (b))                                 // the shared tail's arithmetic: operators, under the kernel's contract(off)
#define QGS_ADD(a, b) ((a) + (b))

struct KSched {
    int32_t n, n_gaits, random_phase, done_row;
    int32_t done_kind, done_stride;
    float freq_lo, span, dt, kappa, inv2k, inv_sf2, inv_sv2, height, min_command_speed, threshold;
    float w[QG_SCHED_NTERMS];
    uint64_t seed_s, base;
    KShapedIO io;
    int32_t obs_stride, obs_dim, out_stride, copy_obs, vec;
    int32_t term_obs_stride, term_out_stride, copy_term, term_vec;
};

// ---- the draws of an episode, on both sides of the launch ------------------------------------------------------------------------------------
__host__ __device__ static inline int32_t qgs_gait(uint64_t key, int32_t n_gaits) { return (int32_t)(((uint64_t)qgp_k(key, 0) * (uint64_t)n_gaits) >> 24); }
__host__ __device__ static inline float qgs_freq(uint64_t key, float freq_lo, float span) {
#pragma clang fp contract(off)
    const float u = (float)qgp_k(key, 1) * 0x1p-24f;              // exact
    const float t = span * u;
    return freq_lo + t;
}
__host__ __device__ static inline uint32_t qgs_phi0(uint64_t key, int32_t random_phase) { return random_phase ? qgp_k(key, 2) << 8 : 0u; }
// freq * dt32 <= 0.5 (checked at the launch): the product of two f32 is exact in f64, and so is the scaling
__host__ __device__ static inline uint32_t qgs_dphi(float freq, float dt) { return (uint32_t)rint((double)freq * (double)dt * 4294967296.0); }

// foot phase q of a schedule with stance D: hard flag, p and s
__device__ __forceinline__ void qgs_foot(const KSched &A, uint32_t q, uint32_t D, bool &hard, float &s) {
#pragma clang fp contract(off)
    hard = q < D;
    const float p = (float)(q >> 8) * 0x1p-24f, d = (float)(D >> 8) * 0x1p-24f;
    const float m = hard ? fminf(p, d - p) : -fminf(p - d, 1.0f - p);
    const float ramp = fminf(fmaxf(0.5f + m * A.inv2k, 0.f), 1.f);
    s = A.kappa == 0.f ? (hard ? 1.f : 0.f) : ramp;
}

// clock column c (0 .. QG_SCHED_DIM - 1) of (phase, gait row, frequency)
__device__ __forceinline__ float qgs_column(const uint32_t *__restrict__ table, int c, uint32_t phi, int32_t g, float freq) {
    const uint32_t *row = table + g * QGS_ROW;
    if (c == QG_SCHED_FREQ) return freq;
    if (c == QG_SCHED_DUTY) return (float)(row[4] >> 8) * 0x1p-24f;
    const uint32_t q = phi + row[c & 3];
    const float two_p = (float)(q >> 8) * 0x1p-23f;               // exact
    return c < QG_SCHED_COS ? sinpif(two_p) : cospif(two_p);
}

// the 16 lanes of a group copy a row of `width` floats
__device__ __forceinline__ void qgs_copy_row(const float *from, float *to, int width, int vec, int lane) {
    if (vec) {
        const float4 *f4 = reinterpret_cast<const float4 *>(from);
        float4 *t4 = reinterpret_cast<float4 *>(to);
        for (int c = lane; c < width / 4; c += 16) t4[c] = f4[c];
    } else {
        for (int c = lane; c < width; c += 16) to[c] = from[c];
    }
}

template <bool DYN>
__global__ __launch_bounds__(QGC_ENVS * 16) void qg_sched_kernel(KSched A, const KModel *__restrict__ M, const float *__restrict__ sq /* [19][n] */,
                                                                 const float *__restrict__ sv /* [18][n] */, const float *__restrict__ dyn,
                                                                 const uint32_t *__restrict__ table, uint32_t *phi_state, int64_t *episode,
                                                                 const void *done, const float *reward, float *reward_out, const float *base,
                                                                 float *comps, const float *command, const float *obs, float *out,
                                                                 const float *term_obs, float *term_out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 15;
    const int64_t e64 = (int64_t)blockIdx.x * QGC_ENVS + (threadIdx.x >> 4);
    if (e64 >= A.n) return;                               // a whole 16-lane group: what is below crosses the lanes of a group only
    const size_t e = (size_t)e64, n = (size_t)A.n;
    const bool live = lane < QG_NBODY;
    const int b = live ? lane : QG_NBODY - 1;             // an idle lane stays in the control flow: body 12 again, nothing stored
    const bool finished = done ? qg_done_at(done, A.done_kind, A.done_stride, e) : false;     // group-uniform

    // ---- lane 0: the env's phase and episode ------------------------------------------------------------------------------------------------
    uint32_t phi_row = 0, phi_old = 0;                    // the row's phase; the old episode's after its advance
    int32_t g_row = 0, g_old = 0;
    float freq_row = 0.f, freq_old = 0.f;
    if (lane == 0) {
        const uint64_t ep = (uint64_t)episode[e];
        const uint64_t key = qgp_key(A.seed_s, A.base + e, ep);
        g_old = qgs_gait(key, A.n_gaits), freq_old = qgs_freq(key, A.freq_lo, A.span);
        phi_old = phi_state[e] + qgs_dphi(freq_old, A.dt);
        phi_row = phi_old, g_row = g_old, freq_row = freq_old;
        uint32_t next = phi_old;
        if (finished) {
            const uint64_t key1 = qgp_key(A.seed_s, A.base + e, ep + 1);
            next = qgs_phi0(key1, A.random_phase);
            if (A.done_row == QG_PERTURB_DONE_ROW_RESET)
                phi_row = next, g_row = qgs_gait(key1, A.n_gaits), freq_row = qgs_freq(key1, A.freq_lo, A.span);
            episode[e] = (int64_t)(ep + 1);
        }
        phi_state[e] = next;
    }
    phi_row = __shfl(phi_row, 0, 16), g_row = __shfl(g_row, 0, 16), freq_row = __shfl(freq_row, 0, 16);
    phi_old = __shfl(phi_old, 0, 16), g_old = __shfl(g_old, 0, 16), freq_old = __shfl(freq_old, 0, 16);

    // ---- the sensor's part: forces, positions, flags; this lane's share of the three summed terms --------------------------------------------
    float x[3], v[3], F[3];
    qgc_body<DYN>(M, sq, sv, dyn, b, e, n, x, v, F);
    bool stand = false;
    if (command) {
        const float *c = command + e * (size_t)A.io.command_stride;
        stand = QG_SHAPED_SPEED(c) <= A.min_command_speed;
    }
    const bool foot = live && b != 0 && (b - 1) % 3 == 2;
    float a_force = 0.f, a_vel = 0.f, a_height = 0.f;
    bool match = false;
    if (foot) {
        const int f = (b - 1) / 3;
        const uint32_t *row = table + g_old * QGS_ROW;    // a live env's row is the old episode's; a finished env's terms are zeros
        bool hard;
        float s;
        qgs_foot(A, phi_old + row[f], row[4], hard, s);
        if (stand) hard = true, s = 1.f;
        const bool contact = F[2] > A.threshold;          // the foot flag's exact f32 comparison
        match = contact == hard;
        const float swing = 1.f - s, lift = x[2] - A.height;
        const float f2 = (F[0] * F[0] + F[1] * F[1]) + F[2] * F[2], v2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
        a_force = swing * (1.f - expf(-f2 * A.inv_sf2));
        a_vel = s * (1.f - expf(-v2 * A.inv_sv2));
        a_height = swing * (lift * lift);
    }

    // ---- the reduction over the 16 lanes of the env: every lane of the group is here ------------------------------------------------------
    float s_force = __shfl(a_force, 3, 16), s_vel = __shfl(a_vel, 3, 16), s_height = __shfl(a_height, 3, 16);
#pragma unroll
    for (int src = 6; src <= 12; src += 3) {               // feet 1, 2, 3: ascending
        s_force = s_force + __shfl(a_force, src, 16), s_vel = s_vel + __shfl(a_vel, src, 16), s_height = s_height + __shfl(a_height, src, 16);
    }
    const unsigned group = (unsigned)(__ballot(match) >> (threadIdx.x & 48)) & 0xffffu;      // the env's 16 flags (set on foot lanes only)
    const float term[QG_SCHED_NTERMS] = {s_force, s_vel, s_height, (float)__popc(group)};
    // ---- the tail of a shaped-reward kernel (qg_shaped_dev.h): comp[], their sum, the component columns and the reward ----------------------
    QG_SHAPED_WEIGH(QG_SCHED_NTERMS, A.w, term, QGS_MUL, QGS_ADD)
    QG_SHAPED_STORE(QG_SCHED_NTERMS, A.io, QGS_ADD)

    // ---- the wide rows: the observation in front, the ten clock columns behind it ---------------------------------------------------------------
    if (out) {
        float *to = out + e * (size_t)A.out_stride;
        if (A.copy_obs) qgs_copy_row(obs + e * (size_t)A.obs_stride, to, A.obs_dim, A.vec, lane);
        if (lane < QG_SCHED_DIM) to[A.obs_dim + lane] = qgs_column(table, lane, phi_row, g_row, freq_row);
    }
    if (term_out && finished) {                            // (QG_PERTURB_DONE_ROW_RESET only: checked at the launch)
        float *to = term_out + e * (size_t)A.term_out_stride;
        if (A.copy_term) qgs_copy_row(term_obs + e * (size_t)A.term_obs_stride, to, A.obs_dim, A.term_vec, lane);
        if (lane < QG_SCHED_DIM) to[A.obs_dim + lane] = qgs_column(table, lane, phi_old, g_old, freq_old);
    }
}

// begin: one thread per env
__global__ __launch_bounds__(256) void qg_sched_begin_kernel(KSched A, const uint32_t *__restrict__ table, uint32_t *phi_state, int64_t *episode,
                                                             const uint8_t *mask, float *rows, int32_t row_stride, int32_t obs_dim) {
    const int64_t e64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e64 >= A.n) return;
    const size_t e = (size_t)e64;
    if (mask && mask[e] == 0) return;
    const uint64_t ep = (uint64_t)episode[e] + 1;
    const uint64_t key = qgp_key(A.seed_s, A.base + e, ep);
    const uint32_t phi = qgs_phi0(key, A.random_phase);
    episode[e] = (int64_t)ep, phi_state[e] = phi;
    if (rows) {
        const int32_t g = qgs_gait(key, A.n_gaits);
        const float freq = qgs_freq(key, A.freq_lo, A.span);
        float *to = rows + e * (size_t)row_stride + obs_dim;
        for (int c = 0; c < QG_SCHED_DIM; ++c) to[c] = qgs_column(table, c, phi, g, freq);
    }
}

// ------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------
struct qg_sched {
    qg_contact *contact;
    qg_sched_desc desc;
    KSched k;                 // the handle's constants of a launch; the call's are filled in per launch
    QgDevMem mem;
    uint32_t *d_phi;          // [n]
    int64_t *d_episode;       // [n]
    uint32_t *d_table;        // [QG_SCHED_MAX_GAITS][QGS_ROW]
};

static int sched_validate(const qg_sched_desc *d) {
    if (!d) return fail(QG_ERR_ARG, "qg_sched_create: null description");
    QG_CHECK_STRUCT(d, qg_sched_desc);
    if (d->reserved != 0) return fail(QG_ERR_ARG, "qg_sched: reserved must be 0");
    if (d->n_gaits < 1 || d->n_gaits > QG_SCHED_MAX_GAITS) return fail(QG_ERR_ARG, "qg_sched: n_gaits %d outside 1 .. %d", d->n_gaits, QG_SCHED_MAX_GAITS);
    if (d->random_phase != 0 && d->random_phase != 1) return fail(QG_ERR_ARG, "qg_sched: random_phase %d must be 0 or 1", d->random_phase);
    if (d->done_row != QG_PERTURB_DONE_ROW_RESET && d->done_row != QG_PERTURB_DONE_ROW_TERMINAL)
        return fail(QG_ERR_ARG, "qg_sched: done_row %d is neither QG_PERTURB_DONE_ROW_RESET nor _TERMINAL", d->done_row);
    if (!qg_finite32(d->freq_lo) || !qg_finite32(d->freq_hi) || !(d->freq_lo > 0.f) || !(d->freq_lo <= d->freq_hi))
        return fail(QG_ERR_ARG, "qg_sched: frequencies (%g, %g) must be finite and satisfy 0 < freq_lo <= freq_hi", d->freq_lo, d->freq_hi);
    if (!qg_finite32(d->kappa) || d->kappa < 0.f || d->kappa > 0x1p-7f) return fail(QG_ERR_ARG, "qg_sched: kappa %g outside 0 .. 1/128", d->kappa);
    if (!qg_finite32(d->sigma_force) || !(d->sigma_force > 0.f)) return fail(QG_ERR_ARG, "qg_sched: sigma_force %g must be finite and > 0", d->sigma_force);
    if (!qg_finite32(d->sigma_velocity) || !(d->sigma_velocity > 0.f))
        return fail(QG_ERR_ARG, "qg_sched: sigma_velocity %g must be finite and > 0", d->sigma_velocity);
    if (!qg_finite32(d->swing_height_target)) return fail(QG_ERR_ARG, "qg_sched: swing_height_target is not finite");
    if (!qg_finite32(d->min_command_speed) || d->min_command_speed < 0.f)
        return fail(QG_ERR_ARG, "qg_sched: min_command_speed %g must be finite and >= 0", d->min_command_speed);
    QG_TRY(qg_check_weights(d->weights, QG_SCHED_NTERMS, "qg_sched"));
    for (int g = 0; g < d->n_gaits; ++g) {
        for (int f = 0; f < 4; ++f)
            if (!qg_finite32(d->gaits[g].offset[f]) || d->gaits[g].offset[f] < 0.f || !(d->gaits[g].offset[f] < 1.f))
                return fail(QG_ERR_ARG, "qg_sched: gaits[%d].offset[%d] %g outside [0, 1)", g, f, d->gaits[g].offset[f]);
        if (!qg_finite32(d->gaits[g].duty) || d->gaits[g].duty < 0x1p-6f || d->gaits[g].duty > 63.f * 0x1p-6f)
            return fail(QG_ERR_ARG, "qg_sched: gaits[%d].duty %g outside 1/64 .. 63/64", g, d->gaits[g].duty);
    }
    return QG_OK;
}

extern "C" int qg_sched_destroy(qg_sched *p) {
    if (p) qg_free_handle(p, p->contact->sim->device);     // launches may still be in flight on a caller's stream
    return QG_OK;
}

// phi = phi0 of the episodes in `ep` (host), to the device
static int sched_upload_phi0(qg_sched *p, const int64_t *ep) {
    const size_t n = (size_t)p->k.n;
    QgHostBuf<uint32_t> phi(n);
    QG_TRY(phi.oom());
    for (size_t i = 0; i < n; i++) phi[i] = qgs_phi0(qgp_key(p->k.seed_s, p->k.base + i, (uint64_t)ep[i]), p->k.random_phase);
    HIP_TRY(hipMemcpy(p->d_phi, phi, n * sizeof(uint32_t), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    return QG_OK;
}

extern "C" int qg_sched_create(qg_contact *contact, const qg_sched_desc *desc, qg_sched **out) {
    if (!out) return fail(QG_ERR_ARG, "qg_sched_create: null output");
    *out = nullptr;
    QG_TRY(sched_validate(desc));
    if (!contact) return fail(QG_ERR_ARG, "qg_sched_create: null contact sensor");
    qg_sim *s = contact->sim;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    qg_sched *p = qg_new_handle<qg_sched>();
    if (!p) return QG_ERR_ALLOC;
    p->contact = contact;
    p->desc = *desc;
    KSched &k = p->k;
    k.n = s->n, k.n_gaits = desc->n_gaits, k.random_phase = desc->random_phase, k.done_row = desc->done_row;
    k.freq_lo = desc->freq_lo, k.span = desc->freq_hi - desc->freq_lo;
    k.kappa = desc->kappa, k.inv2k = desc->kappa > 0.f ? (float)(1.0 / (2.0 * (double)desc->kappa)) : 0.f;
    k.inv_sf2 = (float)(1.0 / ((double)desc->sigma_force * (double)desc->sigma_force));
    k.inv_sv2 = (float)(1.0 / ((double)desc->sigma_velocity * (double)desc->sigma_velocity));
    k.height = desc->swing_height_target, k.min_command_speed = desc->min_command_speed;
    k.seed_s = desc->seed + QGS_SALT, k.base = desc->env_index_base;
    uint32_t table[QG_SCHED_MAX_GAITS * QGS_ROW] = {0};
    for (int g = 0; g < desc->n_gaits; ++g) {
        for (int f = 0; f < 4; ++f) table[g * QGS_ROW + f] = (uint32_t)(uint64_t)rint((double)desc->gaits[g].offset[f] * 4294967296.0);   // mod 2^32
        table[g * QGS_ROW + 4] = (uint32_t)(uint64_t)rint((double)desc->gaits[g].duty * 4294967296.0);
    }
    const size_t n = (size_t)s->n;
    if (p->mem.alloc(p->d_phi, n * sizeof(uint32_t), true) || p->mem.alloc(p->d_episode, n * sizeof(int64_t), true) ||
        p->mem.alloc(p->d_table, sizeof table)) {
        qg_sched_destroy(p);
        return QG_ERR_ALLOC;
    }
    int rc = QG_OK;
    {
        QgHostBuf<int64_t> ep(n);
        rc = ep.oom();
        if (rc == QG_OK) {
            memset(ep.p, 0, n * sizeof(int64_t));
            rc = sched_upload_phi0(p, ep);
        }
    }
    hipError_t e = rc == QG_OK ? hipMemcpy(p->d_table, table, sizeof table, hipMemcpyHostToDevice) : hipSuccess;
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (rc != QG_OK || e != hipSuccess) {
        qg_sched_destroy(p);
        return rc != QG_OK ? rc : fail(QG_ERR_DEVICE, "qg_sched_create: %s", hipGetErrorString(e));
    }
    *out = p;
    return QG_OK;
}

extern "C" int qg_sched_set_weights(qg_sched *p, const float *weights) {
    if (!p || !weights) return fail(QG_ERR_ARG, "qg_sched_set_weights: null argument");
    QG_TRY(qg_check_weights(weights, QG_SCHED_NTERMS, "qg_sched_set_weights"));
    memcpy(p->desc.weights, weights, sizeof p->desc.weights);     // read by the next launch; a captured launch keeps its own copy
    return QG_OK;
}

// rows of `width` floats that are copied to rows of `width + QG_SCHED_DIM`: the strides, and the one overlap that is allowed
static int sched_check_rows(const char *who, const char *in_name, const char *out_name, const float *in, int32_t in_stride, int32_t width,
                            const float *outp, int32_t out_stride, int64_t n, int32_t *copy, int32_t *vec) {
    *copy = 0, *vec = 0;
    if (!in && width != 0 && outp) return fail(QG_ERR_ARG, "%s: obs_dim %d without %s", who, width, in_name);
    if (in && in_stride < width) return fail(QG_ERR_ARG, "%s: %s_stride %d must be >= obs_dim %d", who, in_name, in_stride, width);
    if (!outp) return QG_OK;
    if ((int64_t)out_stride < (int64_t)width + QG_SCHED_DIM)
        return fail(QG_ERR_ARG, "%s: %s_stride %d must be >= obs_dim + %d = %lld", who, out_name, out_stride, QG_SCHED_DIM, (long long)width + QG_SCHED_DIM);
    if (!in || width == 0) return QG_OK;
    if (in == outp && in_stride == out_stride) return QG_OK;                              // in place: only the ten columns are written
    if (qg_rows_overlap(in, in_stride, width, outp, out_stride, width + QG_SCHED_DIM, n))
        return fail(QG_ERR_ARG, "%s: %s and %s overlap (allowed only as the same rows at the same stride)", who, in_name, out_name);
    *copy = 1;
    *vec = (width % 4 == 0 && in_stride % 4 == 0 && out_stride % 4 == 0 && qg_aligned(in, 16) && qg_aligned(outp, 16)) ? 1 : 0;
    return QG_OK;
}

extern "C" int qg_sched_advance_device(qg_sched *p, const void *done, int32_t done_kind, int32_t done_stride, const float *reward, int32_t reward_stride,
                                    float *reward_out, int32_t reward_out_stride, float *components, int32_t components_stride,
                                    const float *base_components, int32_t base_stride, int32_t base_terms, const float *command,
                                    int32_t command_stride, const float *obs, int32_t obs_stride, int32_t obs_dim, float *out, int32_t out_stride,
                                    const float *terminal_obs, int32_t terminal_obs_stride, float *terminal_out, int32_t terminal_out_stride,
                                    void *stream) {
    const char *who = "qg_sched_advance_device";
    if (!p) return fail(QG_ERR_ARG, "%s: null handle", who);
    QG_TRY(qg_check_done(who, done, done_kind, done_stride));
    qg_contact *c = p->contact;
    qg_sim *s = c->sim;
    KSched A = p->k;
    QG_TRY(qg_shaped_io(who, QG_SCHED_NTERMS, reward, reward_stride, reward_out, reward_out_stride, components, components_stride, base_components,
                        base_stride, base_terms, command, command_stride, s->n, &A.io));
    if (obs_dim < 0) return fail(QG_ERR_ARG, "%s: obs_dim %d must be >= 0", who, obs_dim);
    if (terminal_out && p->desc.done_row != QG_PERTURB_DONE_ROW_RESET)
        return fail(QG_ERR_ARG, "%s: terminal_out goes with QG_PERTURB_DONE_ROW_RESET (with _TERMINAL the row is the terminal observation)", who);
    QG_TRY(sched_check_rows(who, "obs", "out", obs, obs_stride, obs_dim, out, out_stride, s->n, &A.copy_obs, &A.vec));
    QG_TRY(sched_check_rows(who, "terminal_obs", "terminal_out", terminal_obs, terminal_obs_stride, obs_dim, terminal_out, terminal_out_stride, s->n,
                            &A.copy_term, &A.term_vec));
    A.dt = (float)(s->model.timestep * s->task.frame_skip);       // the sensor's dt (qgc_args), the task as it stands at this call
    if ((double)p->desc.freq_hi * (double)A.dt > 0.5)
        return fail(QG_ERR_ARG, "%s: freq_hi %g Hz x dt %g s > 0.5: the phase would advance by more than half a period per env-step", who,
                    p->desc.freq_hi, A.dt);
    if (s->res.active) return fail(QG_ERR_ARG, "%s: the resident step mode is on, the state lives in registers (qg_resident_stop first)", who);

    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    qg_note_caller_stream(s, (hipStream_t)stream);               // a later host-pointer call of the simulator waits for this launch
    memcpy(A.w, p->desc.weights, sizeof A.w);
    A.threshold = c->desc.force_threshold;
    A.done_kind = done_kind, A.done_stride = done ? done_stride : 1;
    A.obs_stride = obs_stride, A.obs_dim = obs_dim, A.out_stride = out_stride;
    A.term_obs_stride = terminal_obs_stride, A.term_out_stride = terminal_out_stride;
    const dim3 grid((unsigned)((s->n + QGC_ENVS - 1) / QGC_ENVS)), block(QGC_ENVS * 16);
    if (s->dyn)
        hipLaunchKernelGGL(qg_sched_kernel<true>, grid, block, 0, (hipStream_t)stream, A, (const KModel *)s->d_model, (const float *)s->st.qpos,
                           (const float *)s->st.qvel, (const float *)s->d_dyn, (const uint32_t *)p->d_table, p->d_phi, p->d_episode, done, reward,
                           reward_out, base_components, components, command, obs, out, terminal_obs, terminal_out);
    else
        hipLaunchKernelGGL(qg_sched_kernel<false>, grid, block, 0, (hipStream_t)stream, A, (const KModel *)s->d_model, (const float *)s->st.qpos,
                           (const float *)s->st.qvel, (const float *)nullptr, (const uint32_t *)p->d_table, p->d_phi, p->d_episode, done, reward,
                           reward_out, base_components, components, command, obs, out, terminal_obs, terminal_out);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_sched_begin_device(qg_sched *p, const uint8_t *mask, float *rows, int32_t row_stride, int32_t obs_dim, void *stream) {
    const char *who = "qg_sched_begin_device";
    if (!p) return fail(QG_ERR_ARG, "%s: null handle", who);
    if (obs_dim < 0) return fail(QG_ERR_ARG, "%s: obs_dim %d must be >= 0", who, obs_dim);
    if (rows && (int64_t)row_stride < (int64_t)obs_dim + QG_SCHED_DIM)
        return fail(QG_ERR_ARG, "%s: row_stride %d must be >= obs_dim + %d = %lld", who, row_stride, QG_SCHED_DIM, (long long)obs_dim + QG_SCHED_DIM);
    qg_sim *s = p->contact->sim;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    hipLaunchKernelGGL(qg_sched_begin_kernel, dim3((unsigned)((s->n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p->k,
                       (const uint32_t *)p->d_table, p->d_phi, p->d_episode, mask, rows, row_stride, obs_dim);
    HIP_TRY(hipGetLastError(), QG_ERR_LAUNCH);
    return QG_OK;
}

extern "C" int qg_sched_get_gaits(qg_sched *p, int32_t *gait, float *freq, uint32_t *phi) {
    if (!p) return fail(QG_ERR_ARG, "qg_sched_get_gaits: null handle");
    HIP_TRY(hipSetDevice(p->contact->sim->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);               // a launch may be in flight on a caller's stream
    const size_t n = (size_t)p->k.n;
    QgHostBuf<int64_t> ep(n);
    QG_TRY(ep.oom());
    HIP_TRY(hipMemcpy(ep, p->d_episode, n * sizeof(int64_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    if (phi) HIP_TRY(hipMemcpy(phi, p->d_phi, n * sizeof(uint32_t), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    for (size_t i = 0; i < n; i++) {
        const uint64_t key = qgp_key(p->k.seed_s, p->k.base + i, (uint64_t)ep[i]);
        if (gait) gait[i] = qgs_gait(key, p->k.n_gaits);
        if (freq) freq[i] = qgs_freq(key, p->k.freq_lo, p->k.span);
    }
    return QG_OK;
}

static int sched_fields(const qg_sched *p, QgField *f) {
    const size_t n = (size_t)p->k.n;
    const QgField all[] = {{p->d_phi, n * sizeof(uint32_t)}, {p->d_episode, n * sizeof(int64_t)}};
    const int k = (int)(sizeof all / sizeof all[0]);
    if (f) memcpy(f, all, sizeof all);
    return k;
}
extern "C" int qg_sched_state_bytes(const qg_sched *p, int64_t *bytes) {
    if (!p || !bytes) return fail(QG_ERR_ARG, "qg_sched_state_bytes: null argument");
    QgField f[QG_MAX_FIELDS];
    *bytes = qg_blob_bytes(f, sched_fields(p, f));
    return QG_OK;
}
extern "C" int qg_sched_get_state(qg_sched *p, void *blob) {
    if (!p || !blob) return fail(QG_ERR_ARG, "qg_sched_get_state: null argument");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_out(p->contact->sim, QGS_BLOB, 0, f, sched_fields(p, f), blob);
}
extern "C" int qg_sched_set_state(qg_sched *p, const void *blob) {
    if (!p || !blob) return fail(QG_ERR_ARG, "qg_sched_set_state: null argument");
    QgField f[QG_MAX_FIELDS];
    return qg_blob_in(p->contact->sim, QGS_BLOB, 0, f, sched_fields(p, f), blob, "qg_sched_set_state");
}
