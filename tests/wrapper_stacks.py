"""Scaffolding of tests/test_zz_wrapper_stacks_gpu.py: the device-side VecEnv wrappers stacked in the orders a training run uses, and
the TWIN that states what such a stack means -- the same env class and seed, stepped bare, with the layers' own handle calls
(``Perturbation.perturb_actions`` / ``observe``, ``GaitReward.step``, ``GaitSchedule.begin`` / ``step``, ``CommandCurriculum.begin`` /
``step``, ``PrivilegedState.read``, ``RunningNormalizer.step`` / ``normalize_obs``) made by hand on its rows, in the stack's order, on the
default stream.  The twin calls no wrapper class.

64 envs whose episodes end inside ten steps (``max_time`` 0.05 s), 24 steps: every case sees several episode ends.  The stacks that
hold the command curriculum stand on envs built without ``random_controls`` (the curriculum draws the commands), the others on envs
whose in-kernel sampler draws them.

The NumPy cold path and the device path differ, as the envs document, on a finished env's row: the NumPy row is the reset row, the
device row what the env's ``_zero_finished`` / ``done_row`` says -- the reset stack for the partially observable env, the TERMINAL
observation for the other two (whose reset row is zeros).  A normaliser's statistics see that row, so for those two envs the two paths
part in every normalised column from the first episode end on.  ``Twin(cold=True)`` states the cold path for them: the row is split
into the reset row (zeros in the actor's columns) and the terminal row behind the perturbation, as ``DevicePerturbedVecEnv.step_wait``
hands them on.  Where the gait schedule is in the stack, the terminal row goes through the schedule's launch in the row's place and
comes back with the OLD episode's clock columns behind it; the reset row gets the NEW episode's clock columns, formed on the host from
the draws the launch left (``schedule.clock_columns``: float64 ``sin`` / ``cos`` rounded once), as
``DeviceGaitScheduleVecEnv.step_wait`` does."""
import functools

import numpy as np
import torch

import gait_schedule_reference as GS
import normalize_reference as R

from quadruped_gym_amd._abi import GAIT_TERMS, PRIV_DIM, SCHED_DIM, SCHED_TERMS
from quadruped_gym_amd.curriculum import CommandCurriculum, DeviceCommandCurriculumVecEnv, initial_weights_for
from quadruped_gym_amd.envs.vec_env import QuadrupedVecEnv
from quadruped_gym_amd.envs.walking import REWARD_KEYS, POWalkingQuadrupedVecEnv, WalkingQuadrupedVecEnv
from quadruped_gym_amd.gait import DeviceGaitRewardVecEnv, GaitReward
from quadruped_gym_amd.monitor import RewardMonitor
from quadruped_gym_amd.normalize import DeviceVecNormalize, RunningNormalizer
from quadruped_gym_amd.perturb import DevicePerturbedVecEnv, Perturbation
from quadruped_gym_amd.privileged import DevicePrivilegedVecEnv
from quadruped_gym_amd.schedule import DeviceGaitScheduleVecEnv, GaitSchedule, clock_columns

DEV = torch.device("cuda:0")
N, STEPS = 64, 24
FORCE_THRESHOLD = 1.0                   # the sensor's and the pack's
WALK = dict(random_controls=True, random_init=True, device_commands=True, reset_options={"min_speed": 0.0, "max_speed": 0.5}, max_time=0.05,
            nan_direction=False)
# under the command curriculum: no sampler of the env's own
WALK_CUR = {k: v for k, v in WALK.items() if k not in ("random_controls", "reset_options", "device_commands")}
ENVS = {
    "plain": (QuadrupedVecEnv, dict(reward_fns={"forward": 1.0, "control_cost": -0.1, "alive_bonus": 1.0}, termination_fns={"fall": 0.05},
                                    max_time=0.05)),
    "walk": (WalkingQuadrupedVecEnv, WALK),
    "po": (POWalkingQuadrupedVecEnv, dict(WALK, obs_window=2)),
    "walk-cur": (WalkingQuadrupedVecEnv, WALK_CUR),
    "po-cur": (POWalkingQuadrupedVecEnv, dict(WALK_CUR, obs_window=2)),
}
# the stacks, inside to outside
STACKS = {1: ("perturb", "norm"), 2: ("perturb", "priv", "norm"), 3: ("perturb", "gait", "norm"), 4: ("perturb", "gait", "priv", "norm"),
          5: ("norm", "priv"),
          6: ("perturb", "sched", "norm"), 7: ("sched", "gait", "norm"), 8: ("perturb", "gait", "sched", "priv", "norm"),
          9: ("perturb", "cur", "norm"), 10: ("perturb", "gait", "sched", "cur", "priv", "norm"),
          11: ("perturb", "cur", "gait", "sched", "priv", "norm")}
# ... around each env that accepts them: the normaliser outside the privileged wrapper is refused around the plain env (stack 5 is
# its order), and stack 5 is the packed step's; the schedule and the curriculum need a command, so the walking envs only
CASES = [(1, "plain"), (1, "walk"), (1, "po"), (2, "walk"), (2, "po"), (3, "plain"), (3, "walk"), (3, "po"), (4, "walk"), (4, "po"), (5, "plain"),
         (6, "walk"), (6, "po"), (7, "walk"), (8, "walk"), (8, "po"), (9, "walk"), (9, "po"), (10, "walk"), (10, "po"), (11, "po")]
# noise, bias and a latency of up to one env-step, all non-zero
NOISE, BIAS, ACTION_NOISE, PERTURB_SEED, DELAYS = {"gyro": 0.05, "accel": 0.1}, {"gyro": 0.02}, 0.05, 3, (0, 1)
GAIT_WEIGHTS = {"feet_air_time": 1.0, "feet_slip": -0.1, "feet_clearance": -0.5, "touchdown_speed": -0.05, "feet_contact_force": -0.01,
                "body_contact": -1.0, "flight": -0.5}
GAIT_LIMITS = dict(air_time_target=0.01, clearance_target=0.05, max_contact_force=20.0, min_command_speed=0.1)
PO_COMMAND = 23                         # the command's vx, vy in a partially observable frame
# the gait schedule: the table, frequencies, weights and options of tests/gait_schedule_reference.py, as test_zz_gait_schedule_gpu.py's SCHED_KW
SCHED_SEED = 7
SCHED = dict(gaits=GS.TABLE, freq=GS.FREQ, weights=GS.WEIGHTS, random_phase=True, **GS.LIMITS)
# the command curriculum: OPTIONS of section 6 of test_zz_command_curriculum_gpu.py, and one criterion per kind of term the stack holds
# inside the curriculum.  The thresholds sit inside the spread of the segments' means of the 64 envs: in episodes this short the robots
# are still settling from the spawn height, so of the gait terms ``flight`` is the one that varies (a step's value is 0 or -0.5: no mean
# of 2 or 5 steps equals -0.375), and ``contact_match`` moves in steps of 0.125 per foot (the conditions of
# test_zz_wrapper_stacks_gpu.py print and assert that the kinds of criteria disagree on some segments)
CUR = dict(speed=(0.0, 0.6), bins=(3, 4), initial_speed=(0.0, 0.2), weight_max=8, delta=3, resample_steps=5, min_steps=2, seed=3)
CUR_CRITERIA = {"base": ("progress_direction_reward_local", (1, 0.0)), "gait": ("flight", (1, -0.375)),
                "sched": ("contact_match", (1, 0.125))}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """Bit equality of two float32 arrays (a reward may be NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def make_env(kind, layers=()):
    cls, options = ENVS[kind + "-cur" if "cur" in layers else kind]
    return cls(N, **options)


def actions():
    """``[STEPS, N, 12]`` on the device, the same for every case."""
    return torch.tensor(np.random.default_rng(11).uniform(-1, 1, (STEPS, N, 12)).astype(np.float32)).to(DEV)


def _upload(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy().copy()


def reward_keys(layers, kind):
    """The component columns of a walking env under ``layers`` (the plain env's packed step has none)."""
    if kind == "plain":
        return None
    keys = list(REWARD_KEYS)
    for name in layers:
        keys += list(GAIT_TERMS) if name == "gait" else list(SCHED_TERMS) if name == "sched" else []
    return keys


def criteria(layers):
    """``{reward key: (sense, threshold)}`` of the curriculum of ``layers``: a base term and, where the stack has them inside the
    curriculum, a gait term and a schedule term."""
    inside = layers[:layers.index("cur")]
    kinds = ["base"] + [kind for kind, name in (("gait", "gait"), ("sched", "sched")) if name in inside]
    return {CUR_CRITERIA[kind][0]: CUR_CRITERIA[kind][1] for kind in kinds}


def criteria_rows(layers, kind):
    """``[(column, sense, threshold)]`` of ``criteria(layers)``: the columns of the rows the curriculum reads."""
    keys = reward_keys(layers[:layers.index("cur")], kind)
    return [(keys.index(key), sense, threshold) for key, (sense, threshold) in criteria(layers).items()]


# ---- the stack ------------------------------------------------------------------------------------------------------------------------------
def build_stack(layers, kind):
    """The wrappers of ``layers`` around a fresh env of ``kind``."""
    env = top = make_env(kind, layers)
    for name in layers:
        if name == "perturb":
            step_seconds = float(env.model.opt.timestep) * env.frame_skip
            top = DevicePerturbedVecEnv(top, obs_noise=NOISE, obs_bias=BIAS, action_noise=ACTION_NOISE,
                                        action_latency=(DELAYS[0] * step_seconds, DELAYS[1] * step_seconds), seed=PERTURB_SEED)
        elif name == "gait":
            top = DeviceGaitRewardVecEnv(top, weights=GAIT_WEIGHTS, force_threshold=FORCE_THRESHOLD, gate_on_command=kind == "po", **GAIT_LIMITS)
        elif name == "sched":
            top = DeviceGaitScheduleVecEnv(top, force_threshold=FORCE_THRESHOLD, gate_on_command=kind == "po", seed=SCHED_SEED, **SCHED)
        elif name == "cur":
            top = DeviceCommandCurriculumVecEnv(top, criteria=criteria(layers), **CUR)
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


def curriculum_state(cur):
    """What a ``CommandCurriculum`` holds, as NumPy: the blob, the weights, the counts and the running segments."""
    return {"state": cur.state(), "weights": cur.weights(), "stats": cur.stats(), "bins": cur.bins()}


class StackDriver:
    """``step_tensor`` of a stack into buffers that live as long as the driver, and what each step filled as NumPy arrays.
    ``launch(a, stream)`` is the part a graph captures -- the stack's step and the monitor's record, nothing else --, ``read()`` the
    wait and the copies.  ``static``: the plain env's packed rows are the driver's too (a replay writes where the capture did)."""

    def __init__(self, stack, layers, kind, static=False):
        self.stack, self.layers, self.kind = stack, layers, kind
        z = lambda *shape, **kw: torch.zeros(shape, device=DEV, **kw)
        self.O = bottom(stack).obs_dim
        self.W = stack.obs_dim
        self.term_dim = getattr(stack, "actor_obs_dim", self.W)
        self.cur = layer_of(stack, DeviceCommandCurriculumVecEnv)
        keys = reward_keys(layers, kind)
        self.packed = None
        if kind == "plain":
            self.wide = z(N, self.W) if layers == STACKS[5] else None
            self.static = z(N, self.O + 2) if static else None
        else:
            self.obs, self.rew, self.done, self.comps = z(N, self.W), z(N), z(N, dtype=torch.uint8), z(N, len(keys))
            self.term = z(N, self.term_dim) if kind == "po" else None
            self.monitor = RewardMonitor.for_env(stack)
            assert self.monitor.keys == keys

    def buffers(self):
        """Every buffer a step fills."""
        names = ("wide", "static") if self.kind == "plain" else ("obs", "rew", "done", "comps", "term")
        return [getattr(self, name) for name in names if getattr(self, name) is not None]

    def launch(self, a, stream=None):
        kw = {} if stream is None else {"stream": stream}
        if self.kind == "plain":
            if self.wide is not None:
                kw["wide"] = self.wide
            if self.static is not None:
                kw["packed"] = self.static
            self.packed = self.stack.step_tensor(a, **kw)
            return
        if self.term is not None:
            kw["terminal_obs"] = self.term
        assert self.stack.step_tensor(a, self.obs, self.rew, self.done, components=self.comps, **kw) is None
        self.monitor.record(self.comps, self.rew, self.done, **({} if stream is None else {"stream": stream}))

    def read(self):
        torch.cuda.synchronize()
        if self.kind == "plain":
            packed = self.packed
            out = {"packed": _np(packed), "reward": _np(packed[:, self.O]), "done": _np(packed[:, self.O + 1]) != 0}
            out["obs"] = _np(self.wide) if self.wide is not None else _np(packed[:, :self.O])
            return out
        out = {"obs": _np(self.obs), "reward": _np(self.rew), "done": _np(self.done) != 0, "components": _np(self.comps)}
        if self.term is not None:
            out["terminal_obs"] = _np(self.term)
        if self.cur is not None:
            out["commands"] = _np(self.cur.commands_tensor)
        return out

    def step(self, a, stream=None):
        self.launch(a, stream)
        return self.read()


# ---- the twin -------------------------------------------------------------------------------------------------------------------------------
class Twin:
    """What the stack ``layers`` around an env of ``kind`` means, with the layers' handles called by hand.  ``cold``: the NumPy
    path's meaning of a finished env's row (the module docstring)."""

    def __init__(self, layers, kind, cold=False):
        self.layers, self.kind, self.cold = layers, kind, cold
        self.env = env = make_env(kind, layers)
        self.po, self.packed = kind == "po", kind == "plain"
        self.O = O = env.obs_dim
        z = lambda *shape, **kw: torch.zeros(shape, device=DEV, **kw)
        self.pert = self.gait = self.sched = self.cur = self.priv = self.norm = self.monitor = None
        width, ncomp = O, len(REWARD_KEYS)
        for name in layers:
            if name == "perturb":
                frame, window = (env.FRAME, env.obs_window) if self.po else (O, 1)
                self.pert = Perturbation(N, frame, window, NOISE, BIAS, ACTION_NOISE, DELAYS, reset_action=list(env._sim.task.default_ctrl),
                                         done_row="reset" if self.po else "terminal", seed=PERTURB_SEED, env_index_base=env._sim.env_index_base,
                                         device=env.device)
                self.delayed = z(N, 12)
            elif name == "gait":
                self.gait = GaitReward(env.contact_sensor(FORCE_THRESHOLD), GAIT_WEIGHTS, **GAIT_LIMITS)
                ncomp += len(GAIT_TERMS)
                self.gait_comps = z(N, ncomp)
            elif name == "sched":
                self.sched = GaitSchedule(env.contact_sensor(FORCE_THRESHOLD), done_row="reset" if self.po else "terminal", seed=SCHED_SEED,
                                          env_index_base=env._sim.env_index_base, **SCHED)
                ncomp += len(SCHED_TERMS)
                self.sched_comps = z(N, ncomp)
                self.sched_inner = width
                width += SCHED_DIM
                self.sched_rows = z(N, width)
                self.sched_term = z(N, width) if self.po else None
            elif name == "cur":
                initial = initial_weights_for(CUR["speed"], CUR["bins"], CUR["initial_speed"], CUR["weight_max"])
                self.cur = CommandCurriculum(env._walk, CUR["speed"], CUR["bins"], initial, CUR["weight_max"], CUR["delta"],
                                             CUR["resample_steps"], CUR["min_steps"], criteria_rows(layers, kind), None, CUR["seed"],
                                             env._sim.env_index_base)
                self.commands = z(N, 4)
            elif name == "priv":
                self.priv = env.privileged_state(FORCE_THRESHOLD)
                width += PRIV_DIM
                self.wide = z(N, width)
            else:
                self.norm = RunningNormalizer(N, width, device=env.device)
                self.norm_width = width
                self.term_wide = z(N, width)        # the wide rows that hold narrow terminal rows in their leading columns
        self.W = width
        if not self.packed:
            keys = reward_keys(layers, kind)
            self.narrow, self.rew, self.done = z(N, O), z(N), z(N, dtype=torch.uint8)
            self.base = z(N, len(REWARD_KEYS))
            self.term = z(N, O) if self.po else None
            self.monitor = RewardMonitor(N, keys, device=env.device)

    def _host_commands(self):
        """``commands`` from the walking layer's slots: what no launch of the curriculum has written yet."""
        velocity, heading = self.env.commands()
        self.commands.copy_(_upload(np.concatenate([velocity, heading], axis=1)))

    def reset(self):
        """The rows of the stack's NumPy ``reset()``; ``raw_reset`` keeps them as they stood in front of the normaliser."""
        rows = _upload(self.env.reset())
        for name in self.layers:
            if name == "perturb":
                self.pert.begin(rows=rows)
            elif name == "sched":
                wide = torch.zeros((N, rows.shape[1] + SCHED_DIM), device=DEV)
                wide[:, :rows.shape[1]] = rows
                rows = self.sched.begin(rows=wide)
            elif name == "cur":
                self.cur.begin()
                self._host_commands()
            elif name == "priv":
                wide = torch.empty((N, rows.shape[1] + PRIV_DIM), device=DEV)
                self.priv.read(wide, rows)
                rows = wide
            elif name == "norm":
                self.raw_reset = _np(rows)
                self.norm.reset_returns()
                self.norm.update_obs(rows)
                rows = self.norm.normalize_obs(rows)
        torch.cuda.synchronize()
        return _np(rows)

    def _command(self, rows):
        """The newest frame's (vx, vy): what gates ``feet_air_time`` and the schedule on the partially observable env."""
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

    def _schedule(self, rows, rew, done, term, comps, split):
        """The schedule's launch behind the env-step: ``(rows, term)`` ten columns wider."""
        sched, W = self.sched, self.sched_inner
        if not split:
            sched.step(done, rew, rew, self.sched_comps, comps, self._command(rows), rows, self.sched_rows, term,
                       self.sched_term if term is not None else None)
            return self.sched_rows, self.sched_term if term is not None else None
        # the cold path of a walking env: the terminal row goes through the launch in the row's place ...
        fin = done != 0
        sched.step(done, rew, rew, self.sched_comps, comps, None, torch.where(fin[:, None], term, rows), self.sched_rows)
        wide_term = self.sched_rows.clone()
        # ... and the reset row, as it came from inside, gets the new episode's columns from the draws the launch left
        now = sched.gaits()
        self.sched_rows[:, :W][fin] = rows[fin]
        self.sched_rows[:, W:][fin] = _upload(clock_columns(sched.table, now["gait"], now["freq"], now["phi"]))[fin]
        return self.sched_rows, wide_term

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
        raw, stand = {}, None
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
                    self.gait.step(done, rew, rew, self.gait_comps, comps, self._command(rows))
                    comps = self.gait_comps
            elif name == "sched":
                if self.po:                          # what the gate read: "stand" at or below min_command_speed
                    stand = _np(self._command(rows)[:, :2].abs().amax(dim=1) <= float(np.float32(SCHED["min_command_speed"])))
                rows, term = self._schedule(rows, rew, done, term, comps, split)
                comps = self.sched_comps
            elif name == "cur":
                self.cur.step(done, comps, self.commands)
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
        if self.cur is not None:
            out["commands"] = _np(self.commands)
        if stand is not None:
            out["stand"] = stand
        return out

    def close(self):
        for h in (self.monitor, self.norm, self.pert):
            if h is not None:
                h.close()
        self.env.close()                            # the sensor, the handles bound to it or to the walking layer and the pack are the simulator's children


# ---- one run of a case, shared by the tests that read it ---------------------------------------------------------------------------------
def norm_state(nz):
    sd = nz.state_dict()
    return {k: np.array(v) for k, v in sd.items()}


def contact_timers(snap):
    """The contact timers of a (nested) snapshot, or None where the env has no sensor."""
    while "sim" not in snap:
        snap = snap["env"]
    return snap.get("contact")


def final_state(norm, pert, monitor, timers, sched=None, cur=None):
    return {"norm": norm_state(norm), "perturbation": pert.state() if pert is not None else None,
            "monitor": monitor.state() if monitor is not None else None, "contact": timers,
            "schedule": sched.state() if sched is not None else None, "curriculum": curriculum_state(cur) if cur is not None else None}


def stack_final_state(stack, monitor):
    """``final_state`` of every layer a stack holds."""
    pert, sched = layer_of(stack, DevicePerturbedVecEnv), layer_of(stack, DeviceGaitScheduleVecEnv)
    cur = layer_of(stack, DeviceCommandCurriculumVecEnv)
    return final_state(layer_of(stack, DeviceVecNormalize).normalizer, pert.perturbation if pert is not None else None, monitor,
                       contact_timers(stack.snapshot()), sched.schedule if sched is not None else None,
                       cur.curriculum if cur is not None else None)


def _curriculum_counts(cur):
    """The integers the reference holds too, after a step."""
    bins, stats = cur.bins(), cur.stats()
    return {"weights": cur.weights().ravel().copy(), "episodes": stats["episodes"].ravel().copy(), "successes": stats["successes"].ravel().copy(),
            "bin": bins["bin"], "steps": bins["steps"], "segment": bins["segment"]}


@functools.lru_cache(maxsize=None)
def device_run(stack_id, kind):
    """The stack's device path and its twin over the 24 steps: ``{"stack": [...], "twin": [...]}`` per step, the reset rows, the
    statistics the stack's normaliser reports after every step, the curriculum's integers after the reset and after every step, and
    both final states.  Computed once; leave it unchanged."""
    layers = STACKS[stack_id]
    acts = actions()
    stack, twin = build_stack(layers, kind), Twin(layers, kind)
    driver = StackDriver(stack, layers, kind)
    nz = layer_of(stack, DeviceVecNormalize).normalizer
    cur = driver.cur
    run = {"reset": (stack.reset(), twin.reset()), "stack": [], "twin": [], "stats": [], "curriculum": [], "obs_dim": stack.obs_dim, "O": driver.O,
           "terminal_dim": driver.term_dim, "raw_reset": getattr(twin, "raw_reset", None),
           "dt32": np.float32(np.float64(twin.env.model.opt.timestep) * twin.env.frame_skip), "env_index_base": twin.env._sim.env_index_base}
    if cur is not None:
        run["reset_commands"] = (_np(cur.commands_tensor), _np(twin.commands))
        run["reset_curriculum"] = _curriculum_counts(cur.curriculum)
    for t in range(STEPS):
        a = acts[t].clone()
        run["stack"].append(driver.step(a))
        assert torch.equal(a, acts[t])                          # the caller's actions stay as the policy wrote them
        run["twin"].append(twin.step(acts[t]))
        run["stats"].append(norm_state(nz))
        if cur is not None:
            run["curriculum"].append(_curriculum_counts(cur.curriculum))
    run["final"] = (stack_final_state(stack, getattr(driver, "monitor", None)),
                    final_state(twin.norm, twin.pert, twin.monitor, twin.env.snapshot().get("contact"), twin.sched, twin.cur))
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
