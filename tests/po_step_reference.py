"""One walking / partially observable env-step in f64, composed from the oracles alone: nothing in here comes from the GPU.

TEST INFRASTRUCTURE ONLY.  The chain of one env-step, for a batch of states (qpos, qvel, act, nstep), actions, a task and one model
(or one model per env, for per-env dynamics rows):

1. control   ``WalkingOracle.pre_step`` -- the settling gate on the clock before the step; ``data.ctrl`` is its clip to +-1
2. physics   the C oracle (``oracle.Batch``) stepped with that control: the 33 sensors (lagged by one substep, as the engine leaves
             them), the post-step quaternion, the clock after the step (``nstep`` f64 additions of the timestep)
3. reward    ``WalkingOracle.post_step`` on the ORACLE's sensors: the 11 components
4. frame     ``POOracle.step_env`` on the oracle's sensors, the oracle's quaternion, the clipped control and the command in force

``StepChecker`` keeps the two task oracles' histories (estimator, previous control, filter estimate, frame FIFO) over several
env-steps; ``frame_columns`` is the history-free part (everything of the newest frame but the Euler angles) for rollouts that restart
the chain from the device's STATE at every step.  ``compare_stack`` / ``compare_rewards`` are the comparisons the GPU tests apply;
tests/test_po_step_reference.py proves on the CPU that they pass on the checker's own frames and fail for eight deliberate miswirings.
"""
from __future__ import annotations

import copy
import os

import numpy as np

from oracle import po_oracle as P
from oracle import walking_oracle as W

from helpers import oracle_step_each

FRAME = P.FRAME
TIMESTEP = 0.002
DEFAULT_CTRL = np.array([0.0, 0.0, -0.5] * 4)
# column groups of a frame (po_walking_quad.py:48-56)
GROUPS = {"gyro": slice(0, 3), "accel": slice(3, 6), "angles": slice(6, 9), "body_vel": slice(9, 11), "ctrl": slice(11, 23),
          "command": slice(23, 26)}
# test_po_frames_match_oracle: an f32 filter against an f64 one on EQUAL inputs
ANGLE_EQUAL_INPUTS = 2e-4
# test_walking_rewards_match_oracle: the f32 reward against the f64 one on EQUAL sensors
REWARD_EQUAL_INPUTS = (2e-4, 2e-4)
RATIOS = "fraction of the bound"          # key of the maxima dicts: per entry, the largest error / its bound
EXACT = 1e-6                              # ctrl and command columns, reset frames: f32 rounding of exact values

_CLOCK = np.concatenate([[0.0], np.add.accumulate(np.full(1 << 16, TIMESTEP))])      # strictly sequential f64 additions


def clock(nstep):
    """data.time after ``nstep`` substeps since the reset: that many f64 additions of the timestep (as the engine forms it)."""
    return _CLOCK[np.asarray(nstep, np.int64)]


def sensor_bound(sens, tol):
    """|error| the one-step parity tolerance ``tol`` (TOL["A"] of tests/parity.py) allows on each of the 33 sensors."""
    sens = np.asarray(sens, np.float64)
    bound = tol["obs"][0] + tol["obs"][1] * np.abs(sens)
    bound[..., 12:15] = tol["accel"][0] + tol["accel"][1] * np.abs(sens[..., 12:15])
    return bound


def physics(oracle, models, task, state, ctrl, unlagged=False):
    """Step 2 of the chain.  ``models``: one qg_model, or a sequence with one per env.  Returns a dict: ``sens`` [m,33], ``quat`` [m,4]
    (post-step), ``qpos`` / ``qvel`` / ``act`` / ``nstep`` (post-step), ``done``, ``time`` (the clock after the step) and -- with
    ``unlagged`` -- ``sens_unlagged``: the sensors OF the post-step state (what a kernel that forgot the one-substep lag would show)."""
    qpos, qvel, act, nstep = state
    ctrl = np.asarray(ctrl, np.float64)
    if isinstance(models, (list, tuple)):
        each = oracle_step_each(oracle, models, task, state, ctrl)
        batches = each["batches"]
        out = dict(sens=each["obs"], **{k: each[k] for k in ("done", "qpos", "qvel", "act", "nstep")})
    else:
        b = oracle.Batch(models, task, len(qpos))
        b.set_state(np.asarray(qpos, np.float64), np.asarray(qvel, np.float64), np.asarray(act, np.float64), None, nstep)
        obs, _, done, _ = b.step(ctrl)
        q, v, a, _, ns = b.get_state()
        batches = [b]
        out = dict(sens=obs, done=done, qpos=q, qvel=v, act=a, nstep=ns)
    if unlagged:
        envs = [(b.model, b.envs[j]) for b in batches for j in range(b.n)]
        out["sens_unlagged"] = np.array([oracle.substep(model, type(e).from_buffer_copy(e), np.clip(ctrl[i], -1, 1), want_sensors=True)[0]
                                         for i, (model, e) in enumerate(envs)])
    out["quat"] = out["qpos"][:, 3:7].copy()
    out["time"] = clock(out["nstep"])
    return out


def gated_control(nstep, actions, settling_time, joint_centers=DEFAULT_CTRL):
    """Step 1 without history: (control applied, data.ctrl).  walking_quad.py:142-143 and quadruped.py:160."""
    act = np.array(actions, np.float64, copy=True)
    act[clock(nstep) < settling_time] = joint_centers
    return act, np.clip(act, -1.0, 1.0)


def frame_columns(sens, ctrl, velocity_xy, heading_xy):
    """The newest frame of the chain, Euler angles left at NaN (they need the filter's history): [m, 26]."""
    sens = np.asarray(sens, np.float64)
    fr = np.full((len(sens), FRAME), np.nan)
    fr[:, GROUPS["gyro"]], fr[:, GROUPS["accel"]], fr[:, GROUPS["body_vel"]] = sens[:, 15:18], sens[:, 12:15], sens[:, 30:32]
    fr[:, GROUPS["ctrl"]] = ctrl
    fr[:, 23:25] = velocity_xy
    heading_xy = np.asarray(heading_xy, np.float64)
    fr[:, 25] = np.arctan2(heading_xy[:, 1], heading_xy[:, 0])
    return fr


class StepChecker:
    """The composed chain for m envs over consecutive env-steps.  ``reset()`` is the env's first reset (estimate [1,0,0,0], default
    ctrl, the command in force); every ``step`` starts the physics from the STATE it is given (the tests put the same state into the
    device) and carries the task oracles' histories on."""

    def __init__(self, oracle, m, frame_skip, settling_time=0.0, obs_window=1, unit_zero=True):
        self.oracle, self.m, self.frame_skip, self.window = oracle, m, int(frame_skip), int(obs_window)
        self.dt = TIMESTEP * self.frame_skip
        self.settling = float(settling_time)
        self.walk = W.WalkingOracle(m, self.dt, settling_time=settling_time, unit_zero=unit_zero)
        self.po = P.POOracle(m, self.dt, settling_time, obs_window)
        self.data_ctrl = np.tile(DEFAULT_CTRL, (m, 1))

    def set_commands(self, velocity_xy, heading_xy):
        c = self.walk.controls
        c.velocity[:, :2], c.heading[:, :2] = np.asarray(velocity_xy, np.float64), np.asarray(heading_xy, np.float64)
        for i in range(self.m):
            c._update(i)

    def reset(self):
        """The stack reset() returns: [m, window * 26]."""
        self.walk.reset()
        c = self.walk.controls
        self.data_ctrl = np.tile(DEFAULT_CTRL, (self.m, 1))
        return np.stack([self.po.reset_env(i, DEFAULT_CTRL, np.array([1.0, 0, 0, 0]), c.velocity[i, :2], c.heading[i, :2])
                         for i in range(self.m)])

    def step(self, models, task, state, actions, perturb=None, unlagged=False):
        """One env-step.  ``perturb`` [m,33] is added to the oracle's sensors before the task oracles see them (the sensitivity
        measurement and the checker's own tests).  Returns a dict: the ``physics`` entries plus ``applied``, ``ctrl``, ``comps``
        [m,11], ``reward`` [m], ``flip``, ``stack`` [m, window, 26], ``pre_angles`` [m,3] (the estimate BEFORE this step's filter
        update, as Euler angles) and ``time_before``."""
        assert task.frame_skip == self.frame_skip
        nstep = np.asarray(state[3])
        applied = self.walk.pre_step(clock(nstep), self.data_ctrl, np.asarray(actions, np.float64))
        ctrl = np.clip(applied, -1.0, 1.0)
        out = physics(self.oracle, models, task, state, applied, unlagged=unlagged)
        sens = out["sens"] if perturb is None else out["sens"] + perturb
        total, comps, flip = self.walk.post_step(sens, ctrl)
        c = self.walk.controls
        pre = np.stack([P.to_angles(out["quat"][i] if self.po.alias[i] else self.po.orient[i]) for i in range(self.m)])
        stack = np.stack([self.po.step_env(i, out["time"][i], sens[i], ctrl[i], out["quat"][i], c.velocity[i, :2], c.heading[i, :2])
                          for i in range(self.m)]).reshape(self.m, self.window, FRAME)
        self.data_ctrl = ctrl
        out.update(applied=applied, ctrl=ctrl, comps=comps, reward=total, flip=flip, stack=stack, pre_angles=pre,
                   time_before=clock(nstep), sens_seen=sens)
        return out

    def fork(self):
        """An independent copy of the histories (the oracle library handle is shared)."""
        other = copy.copy(self)
        other.walk, other.po, other.data_ctrl = copy.deepcopy(self.walk), copy.deepcopy(self.po), self.data_ctrl.copy()
        return other


def angle_bound(gyro, tol, dt):
    """Tolerance of the Euler-angle columns for an f32 filter on the DEVICE's sensors against the f64 filter on the oracle's, [m]:

    * ``ANGLE_EQUAL_INPUTS`` -- what test_po_frames_match_oracle allows the f32 filter on equal inputs;
    * ``2 * GAIN_IMU * dt`` -- the filter's correction is ``-gain * g / |g| * dt`` with a UNIT gradient direction: where the
      estimate is aligned with gravity the direction is discontinuous in the accelerometer input, so an accelerometer reading that
      differs within its tolerance can turn the whole step around: at most twice its length;
    * ``dt * (atol + rtol * |gyro|)`` -- the gyro's error, within the obs tolerance, integrated over the step."""
    g = np.linalg.norm(np.asarray(gyro, np.float64), axis=-1)
    return ANGLE_EQUAL_INPUTS + 2.0 * P.GAIN_IMU * dt + dt * (tol["obs"][0] + tol["obs"][1] * g)


def _excess(got, ref, atol, rtol=0.0):
    err = np.abs(np.asarray(got, np.float64) - ref)
    return err, err - (atol + rtol * np.abs(ref))


def _check(err, excess, what, maxima, rows=None):
    if err.size == 0:
        return
    maxima[what] = max(maxima.get(what, 0.0), float(np.nanmax(err)))
    with np.errstate(divide="ignore", invalid="ignore"):                    # the largest error as a fraction of its own bound
        part = np.where(err > 0, err / (err - excess), 0.0)
    ratios = maxima.setdefault(RATIOS, {})
    ratios[what] = max(ratios.get(what, 0.0), float(np.nanmax(part)))
    bad = ~(excess <= 0) & ~(np.isnan(err))
    if bad.any():
        w = np.unravel_index(np.nanargmax(np.where(bad, excess, -np.inf)), err.shape)
        row = int(w[0]) if rows is None else int(np.asarray(rows)[w[0]])
        raise AssertionError(f"{what}: largest excess at env {row}, index {w[1:]}: error {err[w]:.3e}, {excess[w]:.3e} over its bound")


def compare_newest(got, exp, tol, dt, what="frame", angles=True, rows=None, maxima=None):
    """The newest frame ``got`` [k,26] against the checker's ``exp`` [k,26] (``frame_columns`` or the last frame of a ``StepChecker``
    stack): gyro, body velocity within TOL obs, accelerometer within TOL accel, ctrl and command exact to f32 rounding, the Euler
    angles (unless ``angles=False``) within ``angle_bound``.  Returns the per-group maxima (updated in ``maxima`` if given)."""
    maxima = {} if maxima is None else maxima
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert got.shape == exp.shape and got.shape[1] == FRAME, (got.shape, exp.shape)
    cols = np.ones(FRAME, bool)
    cols[GROUPS["angles"]] = angles
    assert np.isfinite(got[:, cols]).all(), f"{what}: a frame value is not finite"
    for name in ("gyro", "body_vel"):
        _check(*_excess(got[:, GROUPS[name]], exp[:, GROUPS[name]], *tol["obs"]), f"{what} {name}", maxima, rows)
    _check(*_excess(got[:, GROUPS["accel"]], exp[:, GROUPS["accel"]], *tol["accel"]), f"{what} accel", maxima, rows)
    for name in ("ctrl", "command"):
        _check(*_excess(got[:, GROUPS[name]], exp[:, GROUPS[name]], EXACT), f"{what} {name}", maxima, rows)
    if angles:
        err = np.abs(got[:, GROUPS["angles"]] - exp[:, GROUPS["angles"]])
        _check(err, err - angle_bound(exp[:, GROUPS["gyro"]], tol, dt)[:, None], f"{what} angles", maxima, rows)
    return maxima


def compare_stack(got, exp, tol, dt, computed=1, what="stack", rows=None, maxima=None):
    """The whole returned stack ``got`` [k, window*26] against the checker's ``exp`` [k, window, 26]: the newest frame LAST.  The
    last ``computed`` frames are frames a step computed (``compare_newest``); every frame before them is the reset frame, which
    holds exact values only (zero sensors, the angles of [1,0,0,0], the default ctrl, the command): equal to ``EXACT``."""
    maxima = {} if maxima is None else maxima
    k, window = exp.shape[0], exp.shape[1]
    got = np.asarray(got, np.float64).reshape(k, window, FRAME)
    first = max(0, window - computed)
    for w in range(window - 1, first - 1, -1):
        compare_newest(got[:, w], exp[:, w], tol, dt, what + (" newest" if w == window - 1 else " previous"), rows=rows, maxima=maxima)
    if first:
        _check(*_excess(got[:, :first].reshape(k, -1), exp[:, :first].reshape(k, -1), EXACT), f"{what} reset frames", maxima, rows)
    return maxima


def reward_bounds(comps, sensitivity, dt):
    """Per-component tolerance [k,11]: test_walking_rewards_match_oracle's (f32 reward against f64 on equal sensors: 2e-4 / 2e-4,
    and for the derived component 10, which divides a difference of f32 sensors by dt, rtol 1e-3 and atol 2e-2 / dt * 1e-3 + 1e-3)
    plus the component's sensitivity [11] to sensors that differ within the one-step parity tolerance."""
    comps = np.asarray(comps, np.float64)
    bound = REWARD_EQUAL_INPUTS[0] + REWARD_EQUAL_INPUTS[1] * np.abs(comps)
    bound[:, 10] = 2e-2 / dt * 1e-3 + 1e-3 + 1e-3 * np.abs(comps[:, 10])
    return bound + np.asarray(sensitivity, np.float64)[None, :]


def direction_bound(sens, tol):
    """Component 2 per env, [k]: w * <unit(vel_xy), unit(command)> and |unit(a) - unit(b)| <= 2 |a - b| / |a|, so a body velocity
    within its tolerance moves the term by at most 2 |w| |tol| / |vel_xy| (and never by more than 2 |w|).  The measured sensitivity
    is the LARGEST over the states, which the one state that barely moves sets; this bound holds every other state to its own."""
    sens = np.asarray(sens, np.float64)
    w = abs(float(W.default_params()["w"][2]))
    moved = np.linalg.norm(sensor_bound(sens, tol)[:, 30:32], axis=1)
    with np.errstate(divide="ignore"):
        return w * np.minimum(2.0, 2.0 * moved / np.linalg.norm(sens[:, 30:32], axis=1))


def compare_rewards(got_comps, got_reward, exp_comps, exp_reward, sensitivity, dt, what="reward", rows=None, maxima=None, sens=None,
                    tol=None):
    """``last_components`` [k,11] and the returned reward [k] against the checker's.  NaN components compare as equal; the reward is
    the f32 sum of its components (as the existing tests state it) and within the sum of the components' bounds of the oracle's.
    With the oracle's sensors ``sens`` [k,33] and ``tol``, component 2 is also held to ``direction_bound`` per env."""
    maxima = {} if maxima is None else maxima
    got_comps, exp_comps = np.asarray(got_comps, np.float64), np.asarray(exp_comps, np.float64)
    got_reward, exp_reward = np.asarray(got_reward, np.float64), np.asarray(exp_reward, np.float64)
    assert np.array_equal(np.isnan(got_comps), np.isnan(exp_comps)), f"{what}: NaN components differ"
    bound = reward_bounds(exp_comps, sensitivity, dt)
    err = np.abs(got_comps - exp_comps)
    for j in range(exp_comps.shape[1]):
        _check(err[:, j:j + 1], (err - bound)[:, j:j + 1], f"{what} component {j}", maxima, rows)
    if sens is not None:
        own = REWARD_EQUAL_INPUTS[0] + REWARD_EQUAL_INPUTS[1] * np.abs(exp_comps[:, 2]) + direction_bound(sens, tol)
        _check(err[:, 2:3], (err[:, 2] - own)[:, None], f"{what} component 2 (per env)", maxima, rows)
    assert np.allclose(got_reward, got_comps.sum(1), rtol=1e-5, atol=1e-4, equal_nan=True), f"{what}: the reward is not the sum of its components"
    err = np.abs(got_reward - exp_reward)[:, None]
    _check(err, err - bound.sum(1, keepdims=True), f"{what} total", maxima, rows)
    return maxima


def reward_sensitivity(checker, models, task, schedule, tol, patterns=8, seed=0):
    """Largest change of every reward component, per env-step of ``schedule`` = [(state, actions), ..], when the oracle's sensors move
    by +- their one-step parity tolerance: ``patterns`` seeded sign patterns, each a chain of its own (component 10 differences two
    steps).  Measured on the oracle ALONE.  Returns ([steps, 11], the unperturbed outputs per step); ``checker`` is left untouched."""
    base = checker.fork()
    outs = [base.step(models, task, st, ac) for st, ac in schedule]
    sens = np.zeros((len(schedule), 11))
    rng = np.random.default_rng(seed)
    for _ in range(patterns):
        chain = checker.fork()
        for k, out in enumerate(outs):
            sign = rng.choice([-1.0, 1.0], size=out["sens"].shape)
            chain.walk.pre_step(out["time_before"], chain.data_ctrl, out["applied"])      # the pre-step part takes no sensors
            _, comps, _ = chain.walk.post_step(out["sens"] + sign * sensor_bound(out["sens"], tol), out["ctrl"])
            chain.data_ctrl = out["ctrl"]
            with np.errstate(invalid="ignore"):
                sens[k] = np.fmax(sens[k], np.nanmax(np.abs(comps - out["comps"]), axis=0))
    return sens, outs


def record(env_var, line):
    """Print ``line``; append it to the file the environment variable names, if it is set."""
    print(line)
    path = os.environ.get(env_var)
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def format_maxima(maxima, indent="    "):
    """The maxima of ``compare_*`` as text, each as ``largest error (largest fraction of its bound)``: keys that start with ``step N``
    one line per step, reward components as one list."""
    ratios = maxima.get(RATIOS, {})
    show = lambda k: f"{maxima[k]:.1e} ({ratios.get(k, 0.0):.2f})"
    lines = {}
    for key in sorted(k for k in maxima if k != RATIOS):
        head, rest = (key[:6], key[7:]) if key.startswith("step ") else ("", key)
        lines.setdefault(head, []).append((rest, key))
    out = []
    for head in sorted(lines):
        comps = [f"reward component {j}" for j in range(11)]
        plain = [f"{rest}={show(key)}" for rest, key in lines[head] if rest not in comps]
        listed = [show(key) for c in comps for rest, key in lines[head] if rest == c]
        if listed:
            plain.append("reward components 0-10=[" + ", ".join(listed) + "]")
        out.append((head + ": " if head else "") + "  ".join(plain))
    return ("\n" + indent).join(out)
