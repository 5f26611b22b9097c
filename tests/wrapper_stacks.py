"""Scaffolding of tests/test_zz_wrapper_stacks_gpu.py: the device-side VecEnv wrappers stacked in the orders a training run uses, and
the TWIN that states what such a stack means -- the same env class and seed, stepped bare, with the layers' own handle calls
(``Perturbation.perturb_actions`` / ``observe``, ``GaitReward.step``, ``PrivilegedState.read``, ``RunningNormalizer.step`` /
``normalize_obs``) made by hand on its rows, in the stack's order, on the default stream.  The twin calls no wrapper class.

64 envs whose episodes end inside ten steps (``max_time`` 0.05 s), 24 steps: every case sees several episode ends.

The NumPy cold path and the device path differ, as the envs document, on a finished env's row: the NumPy row is the reset row, the
device row what the env's ``_zero_finished`` / ``done_row`` says -- the reset stack for the partially observable env, the TERMINAL
observation for the other two (whose reset row is zeros).  A normaliser's statistics see that row, so for those two envs the two paths
part in every normalised column from the first episode end on.  ``Twin(cold=True)`` states the cold path for them: the row is split
into the reset row (zeros in the actor's columns) and the terminal row behind the perturbation, as ``DevicePerturbedVecEnv.step_wait``
hands them on."""
import functools

import numpy as np
import torch

import normalize_reference as R

from quadruped_gym_amd._abi import GAIT_TERMS, PRIV_DIM
from quadruped_gym_amd.envs.vec_env import QuadrupedVecEnv
from quadruped_gym_amd.envs.walking import REWARD_KEYS, POWalkingQuadrupedVecEnv, WalkingQuadrupedVecEnv
from quadruped_gym_amd.gait import DeviceGaitRewardVecEnv, GaitReward
from quadruped_gym_amd.monitor import RewardMonitor
from quadruped_gym_amd.normalize import DeviceVecNormalize, RunningNormalizer
from quadruped_gym_amd.perturb import DevicePerturbedVecEnv, Perturbation
from quadruped_gym_amd.privileged import DevicePrivilegedVecEnv

DEV = torch.device("cuda:0")
N, STEPS = 64, 24
FORCE_THRESHOLD = 1.0                   # the sensor's and the pack's
WALK = dict(random_controls=True, random_init=True, device_commands=True, reset_options={"min_speed": 0.0, "max_speed": 0.5}, max_time=0.05,
            nan_direction=False)
ENVS = {
    "plain": (QuadrupedVecEnv, dict(reward_fns={"forward": 1.0, "control_cost": -0.1, "alive_bonus": 1.0}, termination_fns={"fall": 0.05},
                                    max_time=0.05)),
    "walk": (WalkingQuadrupedVecEnv, WALK),
    "po": (POWalkingQuadrupedVecEnv, dict(WALK, obs_window=2)),
}
# the stacks, inside to outside
STACKS = {1: ("perturb", "norm"), 2: ("perturb", "priv", "norm"), 3: ("perturb", "gait", "norm"), 4: ("perturb", "gait", "priv", "norm"),
          5: ("norm", "priv")}
# ... around each env that accepts them: the normaliser outside the privileged wrapper is refused around the plain env (stack 5 is
# its order), and stack 5 is the packed step's
CASES = [(1, "plain"), (1, "walk"), (1, "po"), (2, "walk"), (2, "po"), (3, "plain"), (3, "walk"), (3, "po"), (4, "walk"), (4, "po"), (5, "plain")]
# noise, bias and a latency of up to one env-step, all non-zero
NOISE, BIAS, ACTION_NOISE, PERTURB_SEED, DELAYS = {"gyro": 0.05, "accel": 0.1}, {"gyro": 0.02}, 0.05, 3, (0, 1)
GAIT_WEIGHTS = {"feet_air_time": 1.0, "feet_slip": -0.1, "feet_clearance": -0.5, "touchdown_speed": -0.05, "feet_contact_force": -0.01,
                "body_contact": -1.0, "flight": -0.5}
GAIT_LIMITS = dict(air_time_target=0.01, clearance_target=0.05, max_contact_force=20.0, min_command_speed=0.1)
PO_COMMAND = 23                         # the command's vx, vy in a partially observable frame


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """Bit equality of two float32 arrays (a reward may be NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make_env(kind):
    cls, options = ENVS[kind]
    return cls(N, **options)


def actions():
    """``[STEPS, N, 12]`` on the device, the same for every case."""
    return torch.tensor(np.random.default_rng(11).uniform(-1, 1, (STEPS, N, 12)).astype(np.float32)).to(DEV)


def _upload(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy().copy()


# ---- the stack ------------------------------------------------------------------------------------------------------------------------------
def build_stack(layers, kind):
    """The wrappers of ``layers`` around a fresh env of ``kind``."""
    env = top = make_env(kind)
    for name in layers:
        if name == "perturb":
            step_seconds = float(env.model.opt.timestep) * env.frame_skip
            top = DevicePerturbedVecEnv(top, obs_noise=NOISE, obs_bias=BIAS, action_noise=ACTION_NOISE,
                                        action_latency=(DELAYS[0] * step_seconds, DELAYS[1] * step_seconds), seed=PERTURB_SEED)
        elif name == "gait":
            top = DeviceGaitRewardVecEnv(top, weights=GAIT_WEIGHTS, force_threshold=FORCE_THRESHOLD, gate_on_command=kind == "po", **GAIT_LIMITS)
        elif name == "priv":
            top = DevicePrivilegedVecEnv(top, force_threshold=FORCE_THRESHOLD)
        else:
            top = DeviceVecNormalize(top)
    return top


def _is_wrapper(obj):
    return hasattr(type(obj), "_snapshot_key")


def layer_of(stack, cls):
    """The wrapper of class ``cls`` in ``stack``, or None."""
    while not isinstance(stack, cls):
        if not _is_wrapper(stack):
            return None
        stack = stack.venv
    return stack


def bottom(stack):
    """The env under the wrappers."""
    while _is_wrapper(stack):
        stack = stack.venv
    return stack


def reward_keys(layers, kind):
    """The component columns of a walking env under ``layers`` (the plain env's packed step has none)."""
    return None if kind == "plain" else list(REWARD_KEYS) + (list(GAIT_TERMS) if "gait" in layers else [])


class StackDriver:
    """``step_tensor`` of a stack into buffers that live as long as the driver, and what each step filled as NumPy arrays."""

    def __init__(self, stack, layers, kind):
        self.stack, self.layers, self.kind = stack, layers, kind
        z = lambda *shape, **kw: torch.zeros(shape, device=DEV, **kw)
        self.O = bottom(stack).obs_dim
        self.W = stack.obs_dim
        self.term_dim = getattr(stack, "actor_obs_dim", self.W)
        keys = reward_keys(layers, kind)
        if kind == "plain":
            self.wide = z(N, self.W) if layers == STACKS[5] else None
        else:
            self.obs, self.rew, self.done, self.comps = z(N, self.W), z(N), z(N, dtype=torch.uint8), z(N, len(keys))
            self.term = z(N, self.term_dim) if kind == "po" else None
            self.monitor = RewardMonitor.for_env(stack)
            assert self.monitor.keys == keys

    def step(self, a):
        if self.kind == "plain":
            packed = self.stack.step_tensor(a, wide=self.wide) if self.wide is not None else self.stack.step_tensor(a)
            torch.cuda.synchronize()
            out = {"packed": _np(packed), "reward": _np(packed[:, self.O]), "done": _np(packed[:, self.O + 1]) != 0}
            out["obs"] = _np(self.wide) if self.wide is not None else _np(packed[:, :self.O])
            return out
        extra = {"terminal_obs": self.term} if self.term is not None else {}
        assert self.stack.step_tensor(a, self.obs, self.rew, self.done, components=self.comps, **extra) is None
        self.monitor.record(self.comps, self.rew, self.done)
        torch.cuda.synchronize()
        out = {"obs": _np(self.obs), "reward": _np(self.rew), "done": _np(self.done) != 0, "components": _np(self.comps)}
        if self.term is not None:
            out["terminal_obs"] = _np(self.term)
        return out


# ---- the twin -------------------------------------------------------------------------------------------------------------------------------
class Twin:
    """What the stack ``layers`` around an env of ``kind`` means, with the layers' handles called by hand.  ``cold``: the NumPy
    path's meaning of a finished env's row (the module docstring)."""

    def __init__(self, layers, kind, cold=False):
        self.layers, self.kind, self.cold = layers, kind, cold
        self.env = env = make_env(kind)
        self.po, self.packed = kind == "po", kind == "plain"
        self.O = O = env.obs_dim
        z = lambda *shape, **kw: torch.zeros(shape, device=DEV, **kw)
        self.pert = self.gait = self.priv = self.norm = self.monitor = None
        width = O
        for name in layers:
            if name == "perturb":
                frame, window = (env.FRAME, env.obs_window) if self.po else (O, 1)
                self.pert = Perturbation(N, frame, window, NOISE, BIAS, ACTION_NOISE, DELAYS, reset_action=list(env._sim.task.default_ctrl),
                                         done_row="reset" if self.po else "terminal", seed=PERTURB_SEED, env_index_base=env._sim.env_index_base,
                                         device=env.device)
                self.delayed = z(N, 12)
            elif name == "gait":
                self.gait = GaitReward(env.contact_sensor(FORCE_THRESHOLD), GAIT_WEIGHTS, **GAIT_LIMITS)
            elif name == "priv":
                self.priv = env.privileged_state(FORCE_THRESHOLD)
                width = O + PRIV_DIM
                self.wide = z(N, width)
            else:
                self.norm = RunningNormalizer(N, width, device=env.device)
                self.norm_width = width
                self.term_wide = z(N, width)        # the wide rows that hold narrow terminal rows in their leading columns
        self.W = width
        if not self.packed:
            keys = reward_keys(layers, kind)
            self.narrow, self.rew, self.done = z(N, O), z(N), z(N, dtype=torch.uint8)
            self.base, self.comps = z(N, len(REWARD_KEYS)), z(N, len(keys))
            self.term = z(N, O) if self.po else None
            self.monitor = RewardMonitor(N, keys, device=env.device)

    def reset(self):
        """The rows of the stack's NumPy ``reset()``."""
        rows = _upload(self.env.reset())
        for name in self.layers:
            if name == "perturb":
                self.pert.begin(rows=rows)
            elif name == "priv":
                wide = torch.empty((N, self.O + PRIV_DIM), device=DEV)
                self.priv.read(wide, rows)
                rows = wide
            elif name == "norm":
                self.norm.reset_returns()
                self.norm.update_obs(rows)
                rows = self.norm.normalize_obs(rows)
        torch.cuda.synchronize()
        return _np(rows)

    def _command(self, rows):
        """The newest frame's (vx, vy): what gates ``feet_air_time`` on the partially observable env."""
        if not self.po:
            return None
        lo = (self.env.obs_window - 1) * self.env.FRAME + PO_COMMAND
        return rows[:, lo:lo + 2]

    def _normalize_terminal(self, term):
        """``term [N, O]`` or ``[N, W]`` in place: ``normalize_obs`` on a wide row that holds it in its leading columns."""
        if term.shape[1] == self.norm_width:
            return self.norm.normalize_obs(term)
        self.term_wide[:, :term.shape[1]].copy_(term)
        self.norm.normalize_obs(self.term_wide)
        return term.copy_(self.term_wide[:, :term.shape[1]])

    def step(self, a):
        """One env-step; what it filled, as the stack's driver reports it, and beside it the ``raw`` rows, reward and terminal rows
        as they stood in front of the normaliser."""
        env, O = self.env, self.O
        acts = self.pert.perturb_actions(a, out=self.delayed) if self.pert is not None else a
        if self.packed:
            packed = env.step_tensor(acts)
            rows, rew, done, term, comps = packed[:, :O], packed[:, O], packed[:, O + 1], None, None
        else:
            extra = {"terminal_obs": self.term} if self.po else {}
            env.step_tensor(acts, self.narrow, self.rew, self.done, components=self.base, **extra)
            rows, rew, done, term, comps = self.narrow, self.rew, self.done, self.term, self.base
        split = self.cold and not self.po           # a finished env's row: the reset row (zeros), its terminal row beside it
        raw = {}
        for k, name in enumerate(self.layers):
            if split and term is None and name != "perturb":
                term = rows[:, :O].clone()
                rows[:, :O][done != 0] = 0.0
            if name == "perturb":
                self.pert.observe(rows, done, terminal_obs=term)
            elif name == "gait":
                if self.packed:
                    self.gait.step(done, rew, rew)
                else:
                    self.gait.step(done, rew, rew, self.comps, self.base, self._command(rows))
                    comps = self.comps
            elif name == "priv":
                self.priv.read(self.wide, rows)
                rows = self.wide
            else:
                raw = {"obs": _np(rows), "reward": _np(rew), "terminal_obs": None if term is None else _np(term)}
                self.norm.step(rows, rew, done)
                if term is not None:
                    self._normalize_terminal(term)
        if self.monitor is not None:
            self.monitor.record(comps, rew, done)
        torch.cuda.synchronize()
        out = {"obs": _np(rows), "reward": _np(rew), "done": _np(done) != 0, "raw": raw}
        if self.packed:
            out["packed"] = _np(packed)
        else:
            out["components"] = _np(comps)
        if term is not None:
            out["terminal_obs"] = _np(term)
        return out

    def close(self):
        for h in (self.monitor, self.norm, self.pert):
            if h is not None:
                h.close()
        self.env.close()                            # the sensor, the gait handle bound to it and the pack are the simulator's children


# ---- one run of a case, shared by the tests that read it ---------------------------------------------------------------------------------
def norm_state(nz):
    sd = nz.state_dict()
    return {k: np.array(v) for k, v in sd.items()}


def contact_timers(snap):
    """The contact timers of a (nested) snapshot, or None where the env has no sensor."""
    while "sim" not in snap:
        snap = snap["env"]
    return snap.get("contact")


def final_state(norm, pert, monitor, timers):
    return {"norm": norm_state(norm), "perturbation": pert.state() if pert is not None else None,
            "monitor": monitor.state() if monitor is not None else None, "contact": timers}


@functools.lru_cache(maxsize=None)
def device_run(stack_id, kind):
    """The stack's device path and its twin over the 24 steps: ``{"stack": [...], "twin": [...]}`` per step, the reset rows, the
    statistics the stack's normaliser reports after every step, and both final states.  Computed once; leave it unchanged."""
    layers = STACKS[stack_id]
    acts = actions()
    stack, twin = build_stack(layers, kind), Twin(layers, kind)
    driver = StackDriver(stack, layers, kind)
    nz = layer_of(stack, DeviceVecNormalize).normalizer
    pert = layer_of(stack, DevicePerturbedVecEnv)
    run = {"reset": (stack.reset(), twin.reset()), "stack": [], "twin": [], "stats": [], "obs_dim": stack.obs_dim, "O": driver.O,
           "terminal_dim": driver.term_dim}
    for t in range(STEPS):
        a = acts[t].clone()
        run["stack"].append(driver.step(a))
        assert torch.equal(a, acts[t])                          # the caller's actions stay as the policy wrote them
        run["twin"].append(twin.step(acts[t]))
        run["stats"].append(norm_state(nz))
    run["final"] = (final_state(nz, pert.perturbation if pert is not None else None, getattr(driver, "monitor", None), contact_timers(stack.snapshot())),
                    final_state(twin.norm, twin.pert, twin.monitor, twin.env.snapshot().get("contact")))
    if getattr(driver, "monitor", None) is not None:
        driver.monitor.close()
    stack.close(), twin.close()
    return run


@functools.lru_cache(maxsize=None)
def cold_run(stack_id, kind):
    """What the NumPy cold path of the case is to return, per step: the device run itself for the partially observable env (whose
    finished rows hold the reset stack on both paths), ``Twin(cold=True)`` for the other two."""
    if kind == "po":
        return device_run(stack_id, kind)["reset"][1], device_run(stack_id, kind)["twin"]
    acts = actions()
    twin = Twin(STACKS[stack_id], kind, cold=True)
    first = twin.reset()
    steps = [twin.step(acts[t]) for t in range(STEPS)]
    twin.close()
    return first, steps


def finished_steps(steps):
    """(the number of env-steps that finished, the steps on which an env finished)."""
    counts = [int(s["done"].sum()) for s in steps]
    return sum(counts), [t for t, c in enumerate(counts) if c]


# ---- the float64 audit of the terminal rows ------------------------------------------------------------------------------------------------
def audit_terminal_rows(got, raw, mean, var, epsilon=1e-8, clip=10.0):
    """The output rule of tests/test_normalize_gpu.py on ``got`` (float32 ``[k, O]``, the stack's normalised terminal rows) against
    normalize_reference's float64 formula on ``raw`` with the LEADING ``O`` entries of the statistics the device reported: every
    element within one float32 ulp, clipped elements exactly at the clip.  Returns (the largest error in ulps, the clipped count)."""
    O = raw.shape[1]
    mean, var = np.asarray(mean)[:O], np.asarray(var)[:O]
    ref = R.apply_f64(raw, mean, var, epsilon)
    over = np.abs(ref) > clip * (1 + 1e-6)
    assert np.all(np.abs(got) <= np.float32(clip))
    assert np.array_equal(got[over], (np.sign(ref[over]) * clip).astype(np.float32)), "clipped elements are not exactly at the clip"
    assert np.array_equal(R.apply(raw, mean, var, epsilon, clip)[over], got[over])
    refc = np.clip(ref, -clip, clip)
    err = np.abs(got.astype(np.float64) - refc) / R.ulp32(refc)
    assert err.max() <= 1.0, f"{err.max():.3f} ulp"
    return float(err.max()), int(over.sum())
