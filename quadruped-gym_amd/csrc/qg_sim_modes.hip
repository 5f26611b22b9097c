// qg_sim_modes.hip -- the simulator's two modes that run the per-env forms of the table-driven step kernels: per-env dynamics
// (rows, range, validation against the model) and external wrenches with the push schedule.  Owns switching them on and off and what
// the per-env kernels read behind the model tables (KModelDyn); which kernels run follows from the two flags (qg_sim_baked,
// qg_sim_per_env in qg_sim.h).  No device code.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qg_sim.h"

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
    for (int c = 0; c < QG_NDYN; c++)
        if (!qg_finite32(row[c])) return fail(QG_ERR_ARG, "%s: %s: column %d is not finite", who, what, c);
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
// The dynamics rows through a host buffer, transposed: [QG_NDYN][n] on the device, [n][QG_NDYN] at the ABI.  `out`: the device's rows;
// `in`: the rows of the envs in `mask` (NULL: all), `in_stride` floats apart (0: the same row for every env, which needs no fetch).
static int dyn_rows_transfer(qg_sim *s, float *out, const float *in, size_t in_stride, const uint8_t *mask) {
    const size_t n = (size_t)s->n, bytes = n * QG_NDYN * sizeof(float);
    QgHostBuf<float> h(n * QG_NDYN);
    QG_TRY(h.oom());
    if (!in || in_stride) HIP_TRY(hipMemcpy(h, s->d_dyn, bytes, hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    if (out)
        for (int c = 0; c < QG_NDYN; c++)
            for (size_t i = 0; i < n; i++) out[i * QG_NDYN + c] = h[c * n + i];
    if (in) {
        for (size_t i = 0; i < n; i++)
            if (!mask || mask[i])
                for (int c = 0; c < QG_NDYN; c++) h[c * n + i] = in[i * in_stride + c];
        HIP_TRY(hipMemcpy(s->d_dyn, h, bytes, hipMemcpyHostToDevice), QG_ERR_DEVICE);
    }
    return QG_OK;
}
// identity rows into the dynamics buffer (with them the per-env kernels compute the shared model's bits)
static int dyn_fill_identity(qg_sim *s) {
    float id[QG_NDYN];
    dyn_identity_row(s, id);
    return dyn_rows_transfer(s, nullptr, id, 0, nullptr);
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
    QG_TRY(qg_retire_and_sync(s));   // steps of the shared model may be in flight on a caller's stream
    const size_t n = (size_t)s->n;
    if (!s->d_dyn && s->mem.alloc(s->d_dyn, n * QG_NDYN * sizeof(float))) return QG_ERR_ALLOC;
    if (!s->d_model_dyn && s->mem.alloc(s->d_model_dyn, sizeof(KModelDyn))) return QG_ERR_ALLOC;
    HIP_TRY(hipMemcpy(&s->d_model_dyn->m, s->d_model, sizeof(KModel), hipMemcpyDeviceToDevice), QG_ERR_DEVICE);
    QG_TRY(dyn_fill_identity(s));
    return model_dyn_upload(s);
}
// switch the mode on: the row buffer (identity rows) and the per-env kernels' model pointer, the table-driven kernels
static int dyn_enable(qg_sim *s, const char *who) {
    if (s->dyn) return QG_OK;
    if (!s->xfrc) QG_TRY(per_env_enable(s, who, "per-env dynamics"));     // (wrench mode runs the per-env kernels already, with identity rows)
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
        QG_TRY(dyn_check_row(s, row, "qg_set_dynamics_range", "lo corner"));
        for (int c = 0; c < QG_NDYN; c++)
            if (c < QG_DYN_PAYLOAD_MASS || c > QG_DYN_PAYLOAD_Z) row[c] = r->hi[c];
        QG_TRY(dyn_check_row(s, row, "qg_set_dynamics_range", "hi corner"));
    }
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    QG_TRY(dyn_enable(s, "qg_set_dynamics_range"));
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
    QG_TRY(qg_retire_and_sync(s));
    return dyn_rows_transfer(s, rows, nullptr, 0, nullptr);
}

extern "C" int qg_set_dynamics(qg_sim *s, const uint8_t *mask, const float *rows) {
    if (!s || !rows) return fail(QG_ERR_ARG, "qg_set_dynamics: null argument");
    const size_t n = (size_t)s->n;
    char what[48];
    for (size_t i = 0; i < n; i++) {
        if (mask && !mask[i]) continue;
        snprintf(what, sizeof what, "env %zu", i);
        QG_TRY(dyn_check_row(s, rows + i * QG_NDYN, "qg_set_dynamics", what));
    }
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    QG_TRY(dyn_enable(s, "qg_set_dynamics"));
    // read-modify-write of the rows: steps (and their auto-reset draws) may be in flight on a caller's stream even when the mode was
    // already on (dyn_enable then returns at once) -- the header's ordering contract
    QG_TRY(qg_retire_and_sync(s));
    return dyn_rows_transfer(s, nullptr, rows, QG_NDYN, mask);
}

extern "C" int qg_clear_dynamics(qg_sim *s) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if (!s->dyn) return QG_OK;
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    HIP_TRY(hipDeviceSynchronize(), QG_ERR_LAUNCH);        // per-env steps may be in flight on a caller's stream
    if (s->xfrc) QG_TRY(dyn_fill_identity(s));       // wrench mode keeps the per-env kernels: identity rows
    s->dyn = 0;
    s->dyn_range_set = 0;
    return QG_OK;
}

// ------------------------------------------------------------------------------------------------------
// external wrenches and the push schedule (include/quadgym.h, QG_NXFRC columns per body)
// ------------------------------------------------------------------------------------------------------
static size_t xfrc_bytes(const qg_sim *s) { return (size_t)s->n * QG_NBODY * QG_NXFRC * sizeof(float); }
// switch wrench mode on: zero rows, no schedule, the per-env kernels (with identity dynamics rows unless that mode is on)
static int xfrc_enable(qg_sim *s, const char *who) {
    if (s->xfrc) return QG_OK;
    if (!s->dyn) QG_TRY(per_env_enable(s, who, "external wrenches"));
    else QG_TRY(qg_retire_and_sync(s));        // per-env steps may be in flight on a caller's stream
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
        for (size_t c = 0; c < w; c++)
            if (!qg_finite32(rows[i * w + c]))
                return fail(QG_ERR_ARG, "qg_set_xfrc: env %zu, body %zu, column %zu is not finite", i, c / QG_NXFRC, c % QG_NXFRC);
    }
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    QG_TRY(xfrc_enable(s, "qg_set_xfrc"));
    // steps may be in flight on a caller's stream even when the mode was already on -- the header's ordering contract
    QG_TRY(qg_retire_and_sync(s));
    if (!mask) {
        HIP_TRY(hipMemcpy(s->d_xfrc, rows, xfrc_bytes(s), hipMemcpyHostToDevice), QG_ERR_DEVICE);
        return QG_OK;
    }
    QgHostBuf<float> h(n * w);
    QG_TRY(h.oom());
    HIP_TRY(hipMemcpy(h, s->d_xfrc, xfrc_bytes(s), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    for (size_t i = 0; i < n; i++)
        if (mask[i]) memcpy(h + i * w, rows + i * w, w * sizeof(float));
    HIP_TRY(hipMemcpy(s->d_xfrc, h, xfrc_bytes(s), hipMemcpyHostToDevice), QG_ERR_DEVICE);
    return QG_OK;
}

extern "C" int qg_set_xfrc_device(qg_sim *s, const float *d_rows, void *stream) {
    if (!s || !d_rows) return fail(QG_ERR_ARG, "qg_set_xfrc_device: null argument");
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    // the first call switches the mode on, which waits for the device (not while a stream is captured)
    if (!s->xfrc) QG_TRY(xfrc_enable(s, "qg_set_xfrc_device"));
    // (the resident kernel cannot run in wrench mode; a stale launch is retired as launch_step does)
    if (s->res.launched) QG_TRY(qg_resident_retire(s));
    const hipStream_t st = (hipStream_t)stream;
    qg_note_caller_stream(s, st);
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
    QG_TRY(qg_retire_and_sync(s));
    HIP_TRY(hipMemcpy(rows, s->d_xfrc, xfrc_bytes(s), hipMemcpyDeviceToHost), QG_ERR_DEVICE);
    return QG_OK;
}

extern "C" int qg_set_push(qg_sim *s, const qg_push_params *p) {
    if (!s) return fail(QG_ERR_ARG, "null handle");
    if (!p) {                       // the schedule off; the rows (and the mode) stay
        if (!s->xfrc) return QG_OK;
        HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
        QG_TRY(qg_retire_and_sync(s));
        s->push = KPush{};
        return model_dyn_upload(s);
    }
    if (p->interval < 1) return fail(QG_ERR_ARG, "qg_set_push: interval %d < 1 env-step", p->interval);
    if (p->duration < 1 || p->duration > p->interval)
        return fail(QG_ERR_ARG, "qg_set_push: duration %d outside 1 .. interval (%d)", p->duration, p->interval);
    if (!(p->probability >= 0.f && p->probability <= 1.f)) return fail(QG_ERR_ARG, "qg_set_push: probability %g outside [0, 1]", (double)p->probability);
    if (!(p->force_min >= 0.f && p->force_min <= p->force_max) || !qg_finite32(p->force_max))
        return fail(QG_ERR_ARG, "qg_set_push: force range [%g, %g] (need 0 <= force_min <= force_max, finite)", (double)p->force_min, (double)p->force_max);
    HIP_TRY(hipSetDevice(s->device), QG_ERR_DEVICE);
    QG_TRY(xfrc_enable(s, "qg_set_push"));
    QG_TRY(qg_retire_and_sync(s));
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
    QG_TRY(qg_retire_and_sync(s));      // steps in wrench mode may be in flight on a caller's stream
    HIP_TRY(hipMemset(s->d_xfrc, 0, xfrc_bytes(s)), QG_ERR_DEVICE);
    s->xfrc = 0;
    s->push = KPush{};
    return model_dyn_upload(s);
}
