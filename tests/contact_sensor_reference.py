"""The definition of what ContactSensor.read reports (include/quadgym.h, "foot-contact sensing"), in NumPy: the ground reaction force
of every body at the state as it stands in memory, the feet's position and velocity, the contact flags and the integer gait timers --
the formulae and nothing cleverer, in float64 or in float32 arithmetic -- and the error budget measured by
tests/test_contact_sensor_reference.py.  No GPU, no torch."""
import numpy as np

NBODY, NFOOT, MAXCP = 13, 4, 12
FEET = (3, 6, 9, 12)
FOOT_COLUMNS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "contact", "touchdown", "liftoff", "phase_time", "last_air_time",
                "last_stance_time")

# ---- the measured error budget (tests/test_contact_sensor_reference.py prints a fresh measurement and fails if it exceeds these) ------
# the largest deviation of the float32 evaluation from the float64 evaluation of the same float32 states, over the 664 states of
# tests/golden/contact_cells.npz, as (atol, rtol): |x32 - x64| <= atol + rtol |x64|.
# Where the sizes come from.  A sample point's height carries ~1e-7 m of rounding (positions up to 1 m, eps 6e-8, three links), which
# the stiffness (2569 N/m per point, up to 12 points) turns into ~3e-4 N; the damper multiplies the point's velocity error (~2e-6 m/s at
# joint rates of 10 rad/s) by up to 400 N s/m: ~1e-3 N.  That is the atol.  While the ramp is not saturated (summed penetration S <
# 0.5 mm) the damping coefficient c = 400 S / 5e-4 carries S's RELATIVE error, 1e-7 / S: 5e-4 for a grazing point 0.2 mm in, and the
# damper term c v_n, which dwarfs the spring there (tens of N against 0.5 N), carries it too -- hence an rtol far above float32's eps.
# The tangential force is at most the normal one times mu, or c times the speed: the same sizes.
# measured: normal |err| <= 1.55e-2 N (at 47.5 N; the largest share of atol + rtol |x64| is 0.60), tangential <= 6.5e-3 N (at 57.0 N;
# share 0.55), foot position 1.33e-7 m (share 0.67), foot velocity 5.7e-7 m/s (share 0.57)
BUDGET_FORCE_NORMAL = (2.0e-3, 5.0e-4)
BUDGET_FORCE_TANGENTIAL = (2.0e-3, 5.0e-4)
BUDGET_FOOT_POS = (2.0e-7, 0.0)
BUDGET_FOOT_VEL = (1.0e-6, 0.0)
MARGIN = 4.0          # a different but equally valid rounding order: contraction into fma, rsqrt against sqrt and divide
                      # (the margin tests/adam_reference.py gives for the same reason)
MARGIN_BAND = 2.0e-6  # m: a sample point this close to the contact margin may be counted on one side in float32 and on the other in float64
MAX_EXCLUDED = 0.005  # share of the (state, body) pairs the flag comparison may leave out


def _snap(R):
    """quat_to_rowmajor of csrc/qg_tables.h: axis-aligned mounts are exact 0 / +-1."""
    R = np.array(R, np.float32)
    for t in (0.0, 1.0, -1.0):
        R[np.abs(R - np.float32(t)) < np.float32(1e-7)] = t
    return R


def _quat_to_mat(q):
    w, x, y, z = (q[..., i] for i in range(4))
    one, two = q.dtype.type(1), q.dtype.type(2)
    return np.stack([np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)], -1),
                     np.stack([two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)], -1),
                     np.stack([two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], -1)], -2)


def constants(model, dtype=np.float64):
    """What the definition reads of a qg_model, in `dtype`.  float32: the device tables of csrc/qg_tables.h (f64 -> f32 once, the
    link mounts as snapped rotation matrices, the ramp as its reciprocal)."""
    T = dtype
    quat = np.array([[model.body_quat[b][i] for i in range(4)] for b in range(NBODY)], np.float64)
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    Q = _quat_to_mat(quat)
    cp = np.zeros((NBODY, MAXCP, 3))
    valid = np.zeros((NBODY, MAXCP), bool)
    for b in range(NBODY):
        for i in range(model.ncp[b]):
            cp[b, i] = [model.cp[b][i][d] for d in range(3)]
            valid[b, i] = True
    return dict(pos=np.array([[model.body_pos[b][d] for d in range(3)] for b in range(NBODY)], T),
                Q=_snap(Q).astype(T) if T == np.float32 else Q, ref=np.array([model.jnt_ref[j] for j in range(12)], T),
                parent=[model.body_parent[b] for b in range(NBODY)], cp=cp.astype(T), valid=valid,
                k=T(model.contact_stiffness), c=T(model.contact_damping), margin=T(model.contact_margin), mu=T(model.contact_friction),
                inv_ramp=T(1.0 / model.contact_ramp), dt_sub=float(model.timestep))


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def evaluate(model, qpos, qvel, rows=None, dtype=np.float64):
    """The definition at the states (qpos [n, 19], qvel [n, 18]) on `model`; `rows` [n, 11]: per-env dynamics rows (friction and the two
    contact scales are read).  Every operation in `dtype`.  Returns a dict:
      force [n, 13, 3]    world-frame ground reaction force per body
      foot_pos, foot_vel [n, 4, 3]
      W [n, 13]           the spring sum;  normal_unclipped [n, 13] = W - c v_n(P) (0 where W == 0)
      under [n, 13, 12]   the sample point is below the contact margin;  gap [n, 13]: the smallest |margin - z| of the body's points"""
    T = dtype
    K = constants(model, T)
    qpos, qvel = np.asarray(qpos, T), np.asarray(qvel, T)
    n = len(qpos)
    one, zero = T(1), T(0)
    quat = qpos[:, 3:7]
    quat = quat * (one / np.sqrt((quat * quat).sum(1, dtype=T)))[:, None]
    x, R = np.zeros((n, NBODY, 3), T), np.zeros((n, NBODY, 3, 3), T)
    v, w = np.zeros((n, NBODY, 3), T), np.zeros((n, NBODY, 3), T)
    x[:, 0], R[:, 0], v[:, 0] = qpos[:, 0:3], _quat_to_mat(quat), qvel[:, 0:3]
    w[:, 0] = np.einsum("nij,nj->ni", R[:, 0], qvel[:, 3:6])
    for b in range(1, NBODY):
        p, j = K["parent"][b], b - 1
        x[:, b] = x[:, p] + np.einsum("nij,j->ni", R[:, p], K["pos"][b])
        A = np.einsum("nij,jk->nik", R[:, p], K["Q"][b])
        ang = qpos[:, 7 + j] - K["ref"][j]
        c, s = np.cos(ang).astype(T), np.sin(ang).astype(T)
        R[:, b, :, 0] = c[:, None] * A[:, :, 0] + s[:, None] * A[:, :, 1]
        R[:, b, :, 1] = c[:, None] * A[:, :, 1] - s[:, None] * A[:, :, 0]
        R[:, b, :, 2] = A[:, :, 2]
        v[:, b] = v[:, p] + _cross(w[:, p], x[:, b] - x[:, p])
        w[:, b] = w[:, p] + R[:, b, :, 2] * qvel[:, 6 + j, None]
    r = np.einsum("nbij,bkj->nbki", R, K["cp"])                     # [n, 13, 12, 3] sample points about the body origin, world axes
    pen = K["margin"] - (x[:, :, None, 2] + r[..., 2])
    under = (pen > zero) & K["valid"][None]
    gap = np.where(K["valid"][None], np.abs(pen), np.inf).min(2)
    pen = np.where(under, pen, zero)
    pensum = pen.sum(2, dtype=T)
    s = (pen[..., None] * r).sum(2, dtype=T)
    kc, cc, mu = K["k"], K["c"], K["mu"]
    if rows is not None:
        rows = np.asarray(rows, T)
        mu, kc, cc = rows[:, 0, None], kc * rows[:, 9, None], cc * rows[:, 10, None]
    active = pensum > zero
    W = kc * pensum
    cdamp = cc * np.minimum(pensum * K["inv_ramp"], one)
    P = s * (one / np.where(active, pensum, one))[..., None]         # centre of pressure about the body origin
    vP = v + _cross(w, P)
    fn0 = W - cdamp * vP[..., 2]
    fn = np.maximum(fn0, zero)
    speed = np.sqrt(vP[..., 0] * vP[..., 0] + vP[..., 1] * vP[..., 1])
    sliding = cdamp * speed > mu * fn
    ct = np.where(sliding, mu * fn / np.where(sliding, speed, one), cdamp)
    force = np.stack([-ct * vP[..., 0], -ct * vP[..., 1], fn], -1)
    force = np.where(active[..., None], force, zero).astype(T)
    feet = list(FEET)
    return dict(force=force, foot_pos=x[:, feet], foot_vel=v[:, feet], W=np.where(active, W, zero), under=under, gap=gap,
                normal_unclipped=np.where(active, fn0, zero), body_pos=x, body_vel=v)


def flags(force, threshold=0.0):
    """[n, 13] bool: F_z > threshold."""
    return np.asarray(force)[..., 2] > threshold


def tolerance(budget, ref, margin=1.0):
    return margin * (budget[0] + budget[1] * np.abs(ref))


def share(err, budget, ref):
    """The largest |err| / (atol + rtol |ref|)."""
    return float((np.abs(err) / tolerance(budget, ref)).max())


def flag_band(ref, threshold=0.0, margin=MARGIN):
    """[n, 13] bool: the (state, body) pairs the flag comparison leaves out -- a sample point within MARGIN_BAND of the contact margin,
    or, where the body touches, the unclipped normal force within the force bound of the threshold."""
    near_margin = ref["gap"] < MARGIN_BAND
    f0 = ref["normal_unclipped"]
    near_threshold = (ref["W"] > 0) & (np.abs(f0 - threshold) < tolerance(BUDGET_FORCE_NORMAL, f0, margin))
    return near_margin | near_threshold


# ---- the gait timers: integers ---------------------------------------------------------------------------------------------------------
class Timers:
    """The per-foot timers of `n` envs in whole env-steps; ``advance(contact [n, 4] bool, done [n] bool or None)`` applies the update
    rule of include/quadgym.h and returns this sample's (touchdown, liftoff) [n, 4] bool."""

    def __init__(self, n):
        self.prev = np.zeros((n, NFOOT), np.int32)
        self.phase = np.zeros((n, NFOOT), np.int32)
        self.last_air = np.zeros((n, NFOOT), np.int32)
        self.last_stance = np.zeros((n, NFOOT), np.int32)
        self.armed = np.zeros(n, np.int32)

    def advance(self, contact, done=None):
        contact = np.asarray(contact).astype(np.int32)
        n = len(contact)
        done = np.zeros(n, bool) if done is None else np.asarray(done).astype(bool)
        touchdown, liftoff = np.zeros((n, NFOOT), bool), np.zeros((n, NFOOT), bool)
        for e in range(n):
            for f in range(NFOOT):
                c = contact[e, f]
                if not self.armed[e] or done[e]:
                    self.phase[e, f], self.last_air[e, f], self.last_stance[e, f] = 1, 0, 0
                elif c == self.prev[e, f]:
                    self.phase[e, f] += 1
                else:
                    if c:
                        self.last_air[e, f], touchdown[e, f] = self.phase[e, f], True
                    else:
                        self.last_stance[e, f], liftoff[e, f] = self.phase[e, f], True
                    self.phase[e, f] = 1
                self.prev[e, f] = c
            self.armed[e] = 1
        return touchdown, liftoff

    def reset(self, mask=None):
        self.armed[:] = np.where(np.ones(len(self.armed), bool) if mask is None else np.asarray(mask).astype(bool), 0, self.armed)

    def times(self, dt):
        """(phase_time, last_air_time, last_stance_time) [n, 4] f32: steps x f32(dt), one rounding."""
        dt = np.float32(dt)
        return tuple((a.astype(np.float32) * dt).astype(np.float32) for a in (self.phase, self.last_air, self.last_stance))


def feet_rows(ref, contact, touchdown, liftoff, times):
    """[n, 4, 12] f32 in the layout of FOOT_COLUMNS."""
    n = len(contact)
    out = np.zeros((n, NFOOT, len(FOOT_COLUMNS)), np.float32)
    out[..., 0:3], out[..., 3:6] = ref["foot_pos"], ref["foot_vel"]
    out[..., 6], out[..., 7], out[..., 8] = contact, touchdown, liftoff
    out[..., 9], out[..., 10], out[..., 11] = times
    return out
