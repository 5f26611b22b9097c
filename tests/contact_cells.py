"""States that put every ground-contact sample point on the floor, and the census of what a pool of states reaches.  No GPU.

A *cell* is (body b, sample point i, depth class): grazing (0.02 .. 0.2 mm below the contact margin: the damper's ramp is not
saturated) or pressed (1 .. 3 mm: saturated).  13 bodies carry 12 + 12 * 8 = 108 points, so there are 216 cells.  Rollouts and randomly
tilted robots leave a third of the points in the air (the FRAME's top corners, two to five points of every link), and the per-point
constants are exactly what differs between the step kernels (literals, packed pairs, LDS tables), so each state here is BUILT:

  1. a body-frame direction u for which point i is the unique lowest of body b's points (every point is an extreme point of its body);
  2. hinges in range;  3. body b's orientation from ``oracle.kinematics`` with the base at identity;
  4. the base quaternion that makes world-up, in body b's axes, equal to u, with a random yaw;
  5. the base height that puts point i at contact_margin - depth;
  6. velocities, activations and actions as tools/make_golden.py: contact_states draws them (one state in three as drawn, one with the
     contact point's velocity steered to a slow approach -- the viscous "stick" branch -- and one at 0.3 of the drawn velocities);
  7. everything rounded to f32 -- the census and every check read the rounded numbers.

(u, hinges) are searched -- random draws among the directions that leave point i most clearance, then a hill climb in which u moves
too -- for a pose in which no other body is pressed in deeper than 6 mm, as in contact_states, and point i is alone on its body;
where the legs do not allow the former (a FRAME corner at a hip mount) the cell is kept with the shallowest pose found and the census
lists it.  A cell gets one pose per velocity style; of three draws of the motion on that pose the generator keeps the one that
detects most of the six 1 mm shifts of cp[b][i] (``shift_excess``), preferring states in which point i is ALONE on its body: there the
centre of pressure is that point and its three coordinates are tested by themselves.

Cull-edge states: for the femur, shin and foot of every leg, the point farthest from the body origin (the shin has two) points
straight down (u = -cp / |cp|) and grazes the floor by 0.02 .. 0.1 mm -- what a bounding-sphere cull with too small a radius would
drop.  The FRAME has none: with one of its four corners straight down the best pose the hinge search finds leaves the leg mounted at
that corner 35 mm below the floor, beyond HARD_DEPTH (no kernel culls the FRAME by a sphere; its corners graze in their own cells).

``census`` reads everything from ``oracle.kinematics`` and the oracle's ``Diag`` over the substeps of ONE env-step: per-point hits, the
points alone on their body, the deepest penetration, and the branches of the contact law every body takes.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "contact_cells.npz")
STEP_VECTORS = os.path.join(HERE, "golden", "step_vectors.npz")

NBODY, FRAME_SKIP, SEED = 13, 4, 20261020
GRAZE, PRESS = 0, 1
DEPTH_NAMES = ("grazing", "pressed")
DEPTH_RANGE = ((0.02e-3, 0.2e-3), (1.0e-3, 3.0e-3))          # what the census accepts for a cell of the class ...
DEPTH_DRAW = ((0.03e-3, 0.19e-3), (1.05e-3, 2.95e-3))        # ... and what the generator draws (f32 rounding moves a point by ~1e-8 m)
EDGE_RANGE, EDGE_DRAW = (0.02e-3, 0.1e-3), (0.03e-3, 0.09e-3)
SOFT_DEPTH, HARD_DEPTH, MAX_DEEP_CELLS = 0.006, 0.020, 40
MIN_GAP = 0.0005                                             # point i of a built state is the lowest of its body by at least this
MIN_ALONE_POINTS, MIN_BRANCH_STATES, MAX_WIDE_SHIFT_POINTS = 60, 4, 11
STYLES = 3                                                   # velocity styles = states kept per cell
BRANCHES = ("ramp below 1", "ramp saturated", "normal force clipped to 0", "slip", "stick")
SHIFTS = [(d, s) for d in range(3) for s in (+1.0, -1.0)]    # +x -x +y -y +z -z
SHIFT_NAMES = ("+x", "-x", "+y", "-y", "+z", "-z")
KIND_CELL, KIND_EDGE = 0, 1
STATE_KEYS = ("qpos", "qvel", "act", "nstep", "actions")
LABEL_KEYS = ("kind", "body", "point", "depth_class")
MARGIN = 2.0                                                 # a kernel sitting at the edge of its own tolerance cannot hide the shift


def body_name(b):
    return "FRAME" if b == 0 else "%s of leg %d" % (("femur", "shin", "foot")[(b - 1) % 3], (b - 1) // 3)


def cell_name(b, i, d):
    return "%s (body %d) point %d, %s" % (body_name(b), b, i, DEPTH_NAMES[d])


def sample_points(model):
    """[13] arrays (ncp, 3): the contact sample points in body axes."""
    return [np.array([[model.cp[b][i][d] for d in range(3)] for i in range(model.ncp[b])]) for b in range(NBODY)]


def point_offsets(model):
    return np.concatenate([[0], np.cumsum([model.ncp[b] for b in range(NBODY)])])


# ---- directions -------------------------------------------------------------------------------------------------------------------
def _sphere(n):
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)


_SPHERE = _sphere(20000)


def lowest_directions(cp, i):
    """Unit directions u (world-up in body axes) for which point i is the unique lowest of `cp`, best first, with the height of the
    second-lowest point above it: those of a 20 000-point sphere that keep at least 60 % of the best clearance (and at least 4 mm)."""
    d = np.delete(cp, i, 0) - cp[i]
    gap = (_SPHERE @ d.T).min(1)
    order = np.argsort(-gap, kind="stable")
    best = gap[order[0]]
    assert best > 0.004, "every sample point is an extreme point of its body"
    keep = order[gap[order] >= max(0.6 * best, 0.004)]
    return _SPHERE[keep], gap[keep]


# ---- placing the robot --------------------------------------------------------------------------------------------------------------
def _quat_of(R):
    """Quaternion (w, x, y, z) of a rotation matrix (body -> world)."""
    t = np.trace(R)
    if t > 0:
        s = 2.0 * np.sqrt(1.0 + t)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        k = int(np.argmax(np.diag(R)))
        a, b = (k + 1) % 3, (k + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[k, k] - R[a, a] - R[b, b])
        q = [0.0] * 4
        q[0] = (R[b, a] - R[a, b]) / s
        q[1 + k] = 0.25 * s
        q[1 + a] = (R[a, k] + R[k, a]) / s
        q[1 + b] = (R[b, k] + R[k, b]) / s
    q = np.array(q)
    return q / np.linalg.norm(q)


def _base_rotation(up_in_base, yaw):
    """Base -> world rotation whose third row is `up_in_base` (world-up in base axes), turned by `yaw` about the vertical."""
    r3 = up_in_base / np.linalg.norm(up_in_base)
    e = np.eye(3)[int(np.argmin(np.abs(r3)))]
    a1 = np.cross(e, r3)
    a1 /= np.linalg.norm(a1)
    A = np.stack([a1, np.cross(r3, a1), r3])
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ A


class Placer:
    """Poses of one robot: where every sample point sits when point i of body b is the lowest of its body along u."""

    def __init__(self, oracle, model):
        self.O, self.model = oracle, model
        self.cps = sample_points(model)
        self.off = point_offsets(model)
        self.lo = np.array([model.jnt_range[j][0] for j in range(12)])
        self.hi = np.array([model.jnt_range[j][1] for j in range(12)])
        self.pad = np.zeros((NBODY, 12, 3))
        self.valid = np.zeros((NBODY, 12), bool)
        for b in range(NBODY):
            self.pad[b, :len(self.cps[b])] = self.cps[b]
            self.valid[b, :len(self.cps[b])] = True
        # the search's own call of qgo_kinematics: buffers and pointers made once
        dp = C.POINTER(C.c_double)
        self._q = np.zeros(19)
        self._q[3] = 1.0
        self._xpos, self._xmat, self._xcom = np.zeros((NBODY, 3)), np.zeros((NBODY, 3, 3)), np.zeros((NBODY, 3))
        self._args = (C.byref(model),) + tuple(x.ctypes.data_as(dp) for x in (self._q, self._xpos, self._xmat, self._xcom))
        self._kin = oracle.lib().qgo_kinematics

    def base_frame_points(self, hinges):
        """(108, 3) sample points in base axes about the base origin (base at identity), and the 13 body -> base rotations."""
        self._q[7:] = hinges
        self._kin(*self._args)
        P = self._xpos[:, None, :] + np.einsum("bkj,bij->bki", self.pad, self._xmat)
        return P[self.valid], self._xmat

    def excess(self, b, i, u, hinges):
        """How far below point i the lowest point of the robot sits (0: nothing is lower), and what `qpos` needs."""
        P, xmat = self.base_frame_points(hinges)
        up = xmat[b] @ u
        z = P @ up
        zi = z[self.off[b] + i]
        return zi - z.min(), (up, zi)

    def cost(self, b, i, u, hinges, depth):
        """(cost, depth of the deepest point).  The cost is 0 when no point of the robot would be pressed in deeper than 0.9 SOFT_DEPTH
        and point i would be alone on its body with 1.5 mm to spare; infinite when it is not the lowest of its body by MIN_GAP."""
        h = self.cps[b] @ u
        gap = np.delete(h, i).min() - h[i]
        if gap < MIN_GAP:
            return np.inf, np.inf
        e, _ = self.excess(b, i, u, hinges)
        return max(0.0, depth + e - 0.9 * SOFT_DEPTH) + 0.3 * max(0.0, depth + 0.0015 - gap), depth + e

    def _search_once(self, b, i, dirs, depth, rng, draws=40, climb=600, free_u=True):
        """(u, hinges, cost, deepest): random draws (u among `dirs`) until the cost is 0; failing that, a hill climb from the best draw
        in which the hinges and -- with `free_u` -- the direction move by shrinking random steps (a direction that leaves point i
        less clearance over its own body often lets the rest of the robot stand clear)."""
        best = None
        for _ in range(draws):
            u = dirs[int(rng.integers(len(dirs)))]
            hinges = rng.uniform(self.lo, self.hi)
            c = self.cost(b, i, u, hinges, depth)
            if best is None or c < best[2]:
                best = (u, hinges, c)
            if c[0] == 0.0:
                break
        u, hinges, c = best
        for k in range(climb):
            if c[0] == 0.0:
                break
            sigma = 0.5 * (1.0 - k / climb) + 0.01
            h2 = np.clip(hinges + rng.normal(size=12) * sigma * (rng.random(12) < 0.4), self.lo, self.hi)
            u2 = u
            if free_u and k % 2:
                u2 = u + rng.normal(size=3) * 0.5 * sigma
                u2 /= np.linalg.norm(u2)
            c2 = self.cost(b, i, u2, h2, depth)
            if c2 < c:
                u, hinges, c = u2, h2, c2
        return u, hinges, c

    def search(self, b, i, dirs, depth, rng, free_u=True, tries=6):
        """(u, hinges, depth of the deepest point): the best of up to `tries` searches; the first that keeps every point within SOFT_DEPTH
        ends them."""
        best = None
        for _ in range(tries):
            r = self._search_once(b, i, dirs, depth, rng, free_u=free_u)
            if best is None or r[2] < best[2]:
                best = r
            if best[2][1] <= SOFT_DEPTH:
                break
        return best[0], best[1], best[2][1]

    def qpos(self, b, i, u, hinges, depth, yaw, xy):
        _, (up, zi) = self.excess(b, i, u, hinges)
        q = np.zeros(19)
        q[0:2] = xy
        q[2] = (self.model.contact_margin - depth) - zi
        q[3:7] = _quat_of(_base_rotation(up, yaw))
        q[7:] = hinges
        return q

    def point_velocity(self, qpos, qvel, b, i):
        """World velocity of sample point i of body b (central difference of the kinematics along qvel)."""
        def at(dt):
            q = np.array(qpos, float)
            q[0:3] += dt * qvel[0:3]
            w = qvel[3:6] * dt
            n = np.linalg.norm(w)
            dq = np.r_[np.cos(n / 2), (np.sin(n / 2) / n) * w] if n > 0 else np.array([1.0, 0, 0, 0])
            a, c = q[3:7], dq
            q[3:7] = [a[0] * c[0] - a[1] * c[1] - a[2] * c[2] - a[3] * c[3], a[0] * c[1] + a[1] * c[0] + a[2] * c[3] - a[3] * c[2],
                      a[0] * c[2] - a[1] * c[3] + a[2] * c[0] + a[3] * c[1], a[0] * c[3] + a[1] * c[2] - a[2] * c[1] + a[3] * c[0]]
            q[7:] += dt * qvel[6:]
            xpos, xmat, _ = self.O.kinematics(self.model, q)
            return xpos[b] + xmat[b] @ self.cps[b][i]
        dt = 1e-6
        return (at(dt) - at(-dt)) / (2 * dt)


def draw_motion(placer, rng, qpos, b, i, style):
    """qvel, act, actions of one state.  Style 0: as tools/make_golden.py: contact_states; 1: the same, with the base's linear velocity
    set so that the contact point approaches the floor at 2 .. 20 mm/s and slides at less than half of that (viscous stick); 2: 0.3
    of style 0's velocities."""
    qvel = rng.normal(size=18) * np.r_[0.2 * np.ones(3), 1.0 * np.ones(3), 3.0 * np.ones(12)]
    act = rng.uniform(-0.5, 0.5, 12)
    actions = rng.uniform(-1.3, 1.3, 12)
    vn, frac, ang = rng.uniform(0.002, 0.02), rng.uniform(0.0, 0.5), rng.uniform(-np.pi, np.pi)
    if style == 1:
        qvel[3:] *= 0.3
        vP = placer.point_velocity(qpos, qvel, b, i)
        qvel[0:3] += np.array([frac * vn * np.cos(ang), frac * vn * np.sin(ang), -vn]) - vP
    elif style == 2:
        qvel *= 0.3
    return qvel, act, actions


# ---- the oracle's step on a state, and what a shifted sample point does to it ------------------------------------------------------------
def task_a(oracle):
    task = oracle.default_task()
    task.use_fall, task.fall_height, task.frame_skip = 1, 0.05, FRAME_SKIP
    return task


def oracle_step(oracle, model, task, s):
    """qpos, qvel, obs (accelerometer columns included) after one env-step from the f32 state `s` = (qpos, qvel, act, nstep, actions)."""
    e = oracle.make_env(s[0], s[1], s[2], nstep=int(s[3]))
    obs, _, _, _ = oracle.step(model, task, e, np.asarray(s[4], np.float64))
    return np.array(e.qpos[:]), np.array(e.qvel[:]), obs


def _ratio(got, ref, tol):
    return float((np.abs(got - ref) / (tol[0] + tol[1] * np.abs(ref))).max())


def step_ratio(a, ref, tol):
    """Largest |a - ref| / (atol + rtol |ref|) over qpos, qvel, obs and the accelerometer, in units of `tol` (the callers pass
    TOL["A"] of tests/parity.py)."""
    rest = np.r_[0:12, 15:33]
    return max(_ratio(a[0], ref[0], tol["qpos"]), _ratio(a[1], ref[1], tol["qvel"]), _ratio(a[2][rest], ref[2][rest], tol["obs"]),
               _ratio(a[2][12:15], ref[2][12:15], tol["accel"]))


class ShiftedModels:
    """The robot with cp[b][i] moved by `size` along +-x, +-y, +-z."""

    def __init__(self, oracle):
        self.O, self.cache = oracle, {}

    def get(self, b, i, size):
        key = (b, i, size)
        if key not in self.cache:
            out = []
            for d, sgn in SHIFTS:
                m = self.O.default_model()
                m.cp[b][i][d] += sgn * size
                out.append(m)
            self.cache = {key: out}                           # one point at a time is all the callers need
        return self.cache[key]


def shift_excess(oracle, shifted, task, s, b, i, tol, size=1e-3):
    """[6]: by how many `tol` the oracle's env-step from state `s` moves when cp[b][i] moves by `size` along +-x, +-y, +-z."""
    ref = oracle_step(oracle, oracle.default_model(), task, s)
    return np.array([step_ratio(oracle_step(oracle, m, task, s), ref, tol) for m in shifted.get(b, i, size)])


# ---- census ---------------------------------------------------------------------------------------------------------------------------
def census(oracle, model, states, frame_skip=FRAME_SKIP, labels=None):
    """What the pool `states` (dict with qpos, qvel, act, nstep, actions) reaches over the substeps of one env-step.

    touch [n][13][12]   the point is below the contact margin in some substep
    alone [n][13][12]   ... and in every substep in which its body touches it is the body's only point below the margin
    hits [13][12]       states per point (the mask `valid` tells the points a body has)
    start_depth [n][13][12]  penetration (margin - z; negative: above) at the state itself
    deepest [n]         the deepest penetration of any point at the state itself
    branch [n][13][5]   the body takes the branch (BRANCHES) in some substep
    With `labels` (kind, body, point, depth_class per state): deep_cells = [(body, point, class, deepest of its states)] above 6 mm."""
    qpos, qvel, act = (np.asarray(states[k], np.float64) for k in ("qpos", "qvel", "act"))
    nstep = np.asarray(states["nstep"])
    ctrl = np.clip(np.asarray(states["actions"], np.float64), -1.0, 1.0)
    cps, n = sample_points(model), len(qpos)
    valid = np.zeros((NBODY, 12), bool)
    for b in range(NBODY):
        valid[b, :model.ncp[b]] = True
    touch = np.zeros((n, NBODY, 12), bool)
    shared = np.zeros((n, NBODY, 12), bool)
    start_depth = np.full((n, NBODY, 12), -np.inf)
    branch = np.zeros((n, NBODY, len(BRANCHES)), bool)
    margin, mu = model.contact_margin, model.contact_friction
    for e_i in range(n):
        e = oracle.make_env(qpos[e_i], qvel[e_i], act[e_i], nstep=int(nstep[e_i]))
        for k in range(frame_skip):
            xpos, xmat, _ = oracle.kinematics(model, np.array(e.qpos[:]))
            _, dg = oracle.substep(model, e, ctrl[e_i], want_diag=True)
            for b in range(NBODY):
                pen = margin - (xpos[b][2] + cps[b] @ xmat[b][2])
                if k == 0:
                    start_depth[e_i, b, :len(pen)] = pen
                under = pen > 0
                W = dg.contact_W[b]
                assert (W > 0) == under.any()
                if not under.any():
                    continue
                touch[e_i, b, :len(pen)] |= under
                if under.sum() > 1:
                    shared[e_i, b, :len(pen)] |= under
                ramp = (W / model.contact_stiffness) / model.contact_ramp      # W = stiffness * summed penetration
                Fx, Fy, Fn = dg.contact_F[b][0], dg.contact_F[b][1], dg.contact_F[b][2]
                branch[e_i, b, 0] |= ramp < 1.0
                branch[e_i, b, 1] |= ramp >= 1.0
                if Fn <= 0.0:
                    branch[e_i, b, 2] = True
                else:
                    # slip: |F_t| = mu F_n by construction (to rounding); stick: the viscous force stays inside the cone
                    slip = np.hypot(Fx, Fy) >= mu * Fn * (1.0 - 1e-9)
                    branch[e_i, b, 3 if slip else 4] = True
    out = dict(touch=touch, alone=touch & ~shared, hits=touch.sum(0), valid=valid, start_depth=start_depth,
               deepest=start_depth.reshape(n, -1).max(1), branch=branch, untouched=int((valid & (touch.sum(0) == 0)).sum()))
    if labels is not None:
        deep = {}
        for e_i in np.flatnonzero(np.asarray(labels["kind"]) == KIND_CELL):
            key = (int(labels["body"][e_i]), int(labels["point"][e_i]), int(labels["depth_class"][e_i]))
            if out["deepest"][e_i] > SOFT_DEPTH:
                deep[key] = max(deep.get(key, 0.0), float(out["deepest"][e_i]))
        out["deep_cells"] = [k + (v,) for k, v in sorted(deep.items())]
    return out


def edge_tilt(oracle, model, qpos, b, i):
    """Angle (rad) between world-down in body b's axes and the direction of its sample point i, in the state `qpos`."""
    cp = sample_points(model)[b][i]
    _, xmat, _ = oracle.kinematics(model, np.asarray(qpos, np.float64))
    return float(np.arccos(np.clip(-xmat[b][2] @ cp / np.linalg.norm(cp), -1.0, 1.0)))


def farthest_points(cp):
    r = np.linalg.norm(cp, axis=1)
    return [int(i) for i in np.flatnonzero(r >= r.max() * (1.0 - 1e-12))]


def edge_cells(model):
    """(body, point) the cull-edge states are tried for: the farthest points of every body (the FRAME's four top corners tie, so do
    two points of a shin).  ``generate`` leaves out those that cannot be built within HARD_DEPTH."""
    cps = sample_points(model)
    return [(b, i) for b in range(NBODY) for i in farthest_points(cps[b])]


# ---- generator ------------------------------------------------------------------------------------------------------------------------
def _f32_state(q, v, a, ns, u):
    return (np.asarray(q, np.float32), np.asarray(v, np.float32), np.asarray(a, np.float32), np.int32(ns), np.asarray(u, np.float32))


def _single(s):
    return {k: np.asarray(x)[None] for k, x in zip(STATE_KEYS, s)}


def generate(oracle, tol, seed=SEED, candidates=3, log=None):
    """The fixture: dict of f32 states (STATE_KEYS) and their labels (LABEL_KEYS), cells first (body, point, class, style), then the
    cull-edge states.  `tol`: TOL["A"] of tests/parity.py, the unit of ``shift_excess``.  Deterministic in `seed`: every
    cell draws from its own stream."""
    model, task = oracle.default_model(), task_a(oracle)
    placer, shifted = Placer(oracle, model), ShiftedModels(oracle)
    dirs_of = {}
    rows, labels = [], []

    def directions(b, i):
        key = (0 if b == 0 else 1 + (b - 1) % 3, i)           # the four legs share their links' points
        if key not in dirs_of:
            dirs_of[key] = lowest_directions(placer.cps[b], i)[0]
        return dirs_of[key]

    def pose(rng, b, i, dirs, lo_hi):
        depth = rng.uniform(*lo_hi)
        u, hinges, _ = placer.search(b, i, dirs, depth, rng)
        return placer.qpos(b, i, u, hinges, depth, rng.uniform(-np.pi, np.pi), rng.uniform(-1, 1, 2))

    def edge_pose(rng, b, i):
        """Point i straight down (u = -cp / |cp|), or None where no hinges keep the rest of the robot within HARD_DEPTH that way."""
        depth = rng.uniform(*EDGE_DRAW)
        down = -placer.cps[b][i] / np.linalg.norm(placer.cps[b][i])
        u, hinges, deepest = placer.search(b, i, down[None], depth, rng, free_u=False)
        if deepest > HARD_DEPTH:
            return None
        return placer.qpos(b, i, u, hinges, depth, rng.uniform(-np.pi, np.pi), rng.uniform(-1, 1, 2))

    def candidate(rng, q, b, i, style):
        v, a, act = draw_motion(placer, rng, q, b, i, style)
        return _f32_state(q, v, a, rng.integers(0, 2000), act)

    for b in range(NBODY):
        for i in range(model.ncp[b]):
            dirs = directions(b, i)
            for d in (GRAZE, PRESS):
                rng = np.random.default_rng([seed, b, i, d])
                for style in range(STYLES):
                    best, q = None, pose(rng, b, i, dirs, DEPTH_DRAW[d])
                    for c in range(candidates):
                        s = candidate(rng, q, b, i, style)
                        cen = census(oracle, model, _single(s))
                        ex = shift_excess(oracle, shifted, task, s, b, i, tol)
                        # most shifts detected, then alone on its body, then within the soft depth, then the largest weakest signal
                        score = (int((ex > MARGIN).sum()), bool(cen["alone"][0, b, i]), bool(cen["deepest"][0] <= SOFT_DEPTH),
                                 float(np.minimum(ex, 10 * MARGIN).min()))
                        if best is None or score > best[0]:
                            best = (score, s)
                    rows.append(best[1])
                    labels.append((KIND_CELL, b, i, d))
                    if log:
                        log("%s style %d: %s" % (cell_name(b, i, d), style, best[0]))
    for b, i in edge_cells(model):
        rng = np.random.default_rng([seed, b, i, 2])
        q = edge_pose(rng, b, i)
        if q is not None:
            rows.append(candidate(rng, q, b, i, 2))
            labels.append((KIND_EDGE, b, i, GRAZE))
    out = {k: np.stack([r[j] for r in rows]) for j, k in enumerate(STATE_KEYS)}
    lab = np.array(labels, np.int32)
    out.update({k: lab[:, j].copy() for j, k in enumerate(LABEL_KEYS)})
    return out


def load(path=FIXTURE):
    return dict(np.load(path))


def cell_index(fix):
    """(body, point, depth class) -> indices of the cell's states in the fixture."""
    out = {}
    for e in np.flatnonzero(fix["kind"] == KIND_CELL):
        out.setdefault((int(fix["body"][e]), int(fix["point"][e]), int(fix["depth_class"][e])), []).append(int(e))
    return out


def shift_coverage(oracle, fix, tol):
    """What the 1 mm shifts of cp[b][i] do to the oracle's step, in units of `tol`: per cell (body, point, class) and per point (body,
    point: its two cells together) the largest excess [6] any of its states shows, and per point the same at 2 mm where it misses
    MARGIN at 1 mm somewhere -> ({cell: [6]}, {point: [6]}, {point: [6]})."""
    task, shifted = task_a(oracle), ShiftedModels(oracle)
    per_cell, one, two = {}, {}, {}
    cells = cell_index(fix)
    state = lambda e: tuple(fix[k][e] for k in STATE_KEYS)
    for (b, i) in sorted({k[:2] for k in cells}):
        for d in (GRAZE, PRESS):
            per_cell[(b, i, d)] = np.max([shift_excess(oracle, shifted, task, state(e), b, i, tol) for e in cells[(b, i, d)]], 0)
        one[(b, i)] = np.maximum(per_cell[(b, i, GRAZE)], per_cell[(b, i, PRESS)])
        if (one[(b, i)] <= MARGIN).any():
            idx = cells[(b, i, GRAZE)] + cells[(b, i, PRESS)]
            two[(b, i)] = np.max([shift_excess(oracle, shifted, task, state(e), b, i, tol, 2e-3) for e in idx], 0)
    return per_cell, one, two
