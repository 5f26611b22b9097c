"""The definition of what PrivilegedState.read reports (include/quadgym.h, "privileged state pack"), in NumPy: the 85 columns at the
state as it stands in memory -- the formulae and nothing cleverer, in float64 or in float32 arithmetic in the stated order -- the push
schedule restated in exact integers, and the error budget of the two rotated columns measured by tests/test_privileged_reference.py.
The ground forces and body positions are contact_sensor_reference.evaluate's.  No GPU, no torch."""
import numpy as np

import contact_sensor_reference as CR

DIM = 85
# (name, first column, width) in column order: QG_PRIV_* of include/quadgym.h
COLUMNS = (("base_lin_vel", 0, 3), ("base_ang_vel", 3, 3), ("gravity_dir", 6, 3), ("base_height", 9, 1), ("joint_pos", 10, 12),
           ("joint_vel", 22, 12), ("act", 34, 12), ("foot_contact", 46, 4), ("foot_force", 50, 12), ("foot_height", 62, 4),
           ("body_contact", 66, 1), ("dynamics", 67, 11), ("frame_wrench", 78, 6), ("episode_time", 84, 1))
COL = {name: slice(first, first + width) for name, first, width in COLUMNS}
# columns that are bit copies of what qg_get_state / qg_get_dynamics / qg_get_xfrc return (frame_wrench: while no push is scheduled)
COPIES = ("base_ang_vel", "base_height", "joint_pos", "joint_vel", "act", "dynamics")
NON_FOOT = [b for b in range(CR.NBODY) if b not in CR.FEET]

# ---- the measured error budget (tests/test_privileged_reference.py prints a fresh measurement and fails if it exceeds these) ------------
# the largest deviation of the float32 evaluation from the float64 evaluation of the same float32 states, over the 664 states of
# tests/golden/contact_cells.npz and the seeded pool below (random base orientations, base speeds up to 2 m/s), as (atol, rtol):
# |x32 - x64| <= atol + rtol |x64|.
# Where the sizes come from.  The reciprocal norm carries ~1.5 eps (eps = 6e-8: the sum, the root, the divide), each normalised
# component that and its own rounding, a product of two ~4 eps, and an entry of R0 is built of up to four such products, doubled: up
# to ~10 eps = 6e-7, which is gravity_dir's error.  base_lin_vel is a three-term sum of such entries times speeds of up to 2 m/s: the
# entries' errors partly cancel in the sum (the rows of R0 stay orthogonal to first order), what is left scales with the speed -- hence
# the rtol -- and the atol covers the components that cancel to a small value.
# measured: gravity_dir |err| <= 5.9e-7 (share 0.59), base_lin_vel |err| <= 6.7e-7 m/s (at 1.83 m/s; share 0.59)
BUDGET_GRAVITY_DIR = (1.0e-6, 0.0)
BUDGET_BASE_LIN_VEL = (7.0e-7, 3.0e-7)
POOL_SEED, POOL_SIZE, POOL_SPEED = 20261021, 2048, 2.0


def pool(seed=POOL_SEED, n=POOL_SIZE):
    """(qpos [n, 19], qvel [n, 18]) float32: uniformly random base orientations (quaternions left un-normalised by up to 1e-3, as an
    integrated state is), base velocities of up to POOL_SPEED m/s in random directions, hinges and rates in their usual ranges."""
    rng = np.random.default_rng(seed)
    qpos, qvel = np.zeros((n, 19)), np.zeros((n, 18))
    quat = rng.normal(size=(n, 4))
    quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    qpos[:, 3:7] = quat * (1.0 + rng.uniform(-1e-3, 1e-3, (n, 1)))
    qpos[:, 0:3] = rng.uniform(-1, 1, (n, 3)) + [0, 0, 1.5]
    qpos[:, 7:] = rng.uniform(-0.8, 0.8, (n, 12))
    v = rng.normal(size=(n, 3))
    qvel[:, 0:3] = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0, POOL_SPEED, (n, 1))
    qvel[:, 3:] = rng.uniform(-5, 5, (n, 15))
    return qpos.astype(np.float32), qvel.astype(np.float32)


# ---- the push schedule: exact integers up to the force ------------------------------------------------------------------------------------
MASK = (1 << 64) - 1
C_STREAM, C_ENV, C_COUNTER = 0xA0761D6478BD642F, 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
STREAM_PUSH = 32


def _mix64(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & MASK
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & MASK
    return x ^ (x >> 31)


def bits24(seed, env_index, counter, stream):
    """The 24-bit integer behind the uniform of `stream` of the (seed, env_index, counter) key (Python integers: exact)."""
    x = (int(seed) + C_STREAM * int(stream) + C_ENV * (int(env_index) + 1) + C_COUNTER * (int(counter) + 1)) & MASK
    return _mix64(_mix64(x)) >> 40


def push_window(push, seed, env_index, episode, w):
    """Window w of the schedule `push` ({"interval", "duration", "probability", "force": (lo, hi)}) for the key: None where the window
    holds no push, else (o, k_mag, k_head): the push is active at offsets o <= j < o + duration; the integers behind u_mag, u_head."""
    st = STREAM_PUSH + 4 * int(w)
    # u_gate < probability with u = k / 2^24 exact in f32 and probability an f32: an exact comparison
    if not bits24(seed, env_index, episode, st) / 16777216.0 < float(np.float32(push["probability"])):
        return None
    o = (bits24(seed, env_index, episode, st + 1) * (push["interval"] - push["duration"] + 1)) >> 24
    return o, bits24(seed, env_index, episode, st + 2), bits24(seed, env_index, episode, st + 3)


def push_force(push, seed, env_index, episode, s, dtype=np.float64):
    """The force (fx, fy) on the FRAME at env-step s of the episode; (0, 0) where none is active.  float32: F = fma(hi - lo, u, lo),
    th = f32(2 pi) u, as written (the device's sin / cos are its own polynomials: a few ulp of F away)."""
    T = dtype
    if push is None or push["interval"] <= 0:
        return T(0), T(0)
    w, j = divmod(int(s), push["interval"])
    win = push_window(push, seed, env_index, episode, w)
    if win is None or not win[0] <= j < win[0] + push["duration"]:
        return T(0), T(0)
    lo, hi = (T(np.float32(x)) for x in push["force"])
    u_mag, u_head = T(win[1]) * T(2.0 ** -24), T(win[2]) * T(2.0 ** -24)
    if T == np.float32:
        F = np.float32(np.float64(hi - lo) * np.float64(u_mag) + np.float64(lo))      # one rounding: the product is exact in f64
    else:
        F = lo + (hi - lo) * u_mag
    th = T(6.283185307179586) * u_head
    return T(F * np.cos(th)), T(F * np.sin(th))


# what the device's force may differ by from push_force(float64): F (<= hi) carries 1 ulp, the angle th <= 2 pi carries the rounding
# of f32(2 pi) u (2 pi eps / 2 = 3.8e-7 rad) and the device's sincos polynomial a few ulp of 1: (6e-8 + 3.8e-7 + 4 x 6e-8) hi < 1e-6 hi
PUSH_RTOL = 1.0e-6


def identity_dynamics_row(model):
    row = np.ones(11, np.float32)
    row[0] = np.float32(model.contact_friction)
    row[1:5] = 0
    return row


def base_columns(qpos, qvel, dtype=np.float64):
    """(base_lin_vel [n, 3], gravity_dir [n, 3]) in `dtype`: R0 as contact_sensor_reference forms it, R0^T v summed in column order."""
    T = dtype
    qpos, qvel = np.asarray(qpos, T), np.asarray(qvel, T)
    quat = qpos[:, 3:7]
    quat = quat * (T(1) / np.sqrt((quat * quat).sum(1, dtype=T)))[:, None]
    R = CR._quat_to_mat(quat)
    v = qvel[:, 0:3]
    lin = np.stack([(R[:, 0, d] * v[:, 0] + R[:, 1, d] * v[:, 1]) + R[:, 2, d] * v[:, 2] for d in range(3)], -1)
    return lin.astype(T), (-R[:, 2, :]).astype(T)


def evaluate(model, qpos, qvel, act, nstep, rows=None, wrench=None, threshold=0.0, dtype=np.float64):
    """The 85 columns [n, 85] in `dtype` at the states; `rows` [n, 11]: the envs' dynamics rows (None: the identity row),
    `wrench` [n, 6]: the FRAME's wrench of the next env-step, push included (None: zeros).  Also returns the sensor's reference dict."""
    T = dtype
    n = len(qpos)
    ref = CR.evaluate(model, qpos, qvel, rows=rows, dtype=T)
    out = np.zeros((n, DIM), T)
    out[:, COL["base_lin_vel"]], out[:, COL["gravity_dir"]] = base_columns(qpos, qvel, T)
    out[:, COL["base_ang_vel"]] = np.asarray(qvel)[:, 3:6]
    out[:, COL["base_height"]] = np.asarray(qpos)[:, 2:3]
    out[:, COL["joint_pos"]], out[:, COL["joint_vel"]] = np.asarray(qpos)[:, 7:19], np.asarray(qvel)[:, 6:18]
    out[:, COL["act"]] = act
    flags = CR.flags(ref["force"], T(threshold))
    feet = list(CR.FEET)
    out[:, COL["foot_contact"]] = flags[:, feet]
    out[:, COL["foot_force"]] = ref["force"][:, feet].reshape(n, 12)
    out[:, COL["foot_height"]] = ref["foot_pos"][..., 2]
    out[:, COL["body_contact"]] = flags[:, NON_FOOT].sum(1, keepdims=True)
    out[:, COL["dynamics"]] = identity_dynamics_row(model)[None] if rows is None else rows
    if wrench is not None:
        out[:, COL["frame_wrench"]] = wrench
    out[:, COL["episode_time"]] = episode_time(model, nstep)[:, None]
    return out, ref


def episode_time(model, nstep):
    """f32(nstep) * f32(timestep), one rounding."""
    return (np.asarray(nstep).astype(np.float32) * np.float32(model.timestep)).astype(np.float32)
