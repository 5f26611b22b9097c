"""``GaitSchedule`` and ``DeviceGaitScheduleVecEnv`` -- a commanded gait schedule on rows that stay on the GPU (``qg_sched_*`` of
``include/quadgym.h``, ``csrc/qg_sched.hip``): a phase oscillator per env with a gait (which foot stands when) and a stepping
frequency drawn per episode, shown to the policy as ten clock columns behind the observation -- ``sin`` and ``cos`` of the four feet's
phases, the frequency, the duty factor -- and held by four reward terms: ``swing_force``, ``stance_velocity``, ``swing_height`` and
``contact_match``, weighted, added to the env's reward and written as component columns behind the env's own.

One launch of hand-written gfx950 code behind the env-step.  Forces, foot kinematics and contact flags are the contact sensor's own
device code on the simulator's state; the sensor's timers are neither read nor written, so the launch composes with
``GaitReward.step`` and ``ContactSensor.read`` in any order.  PyTorch is plumbing only; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import functools
import json
import os

import numpy as np

from . import _abi, shaped
from ._abi import SCHED_DIM, SCHED_MAX_GAITS, SCHED_TERMS, QgSchedDesc, check
from ._abi import SCHED_MAX_BASE_TERMS, QgSchedGait                            # (re-exported: names this module has always had)
from .envs.device_wrapper import STEP_BUFFERS, DeviceVecEnvWrapper, stack_layer
from .envs.device_wrapper import stack_layers                                  # (re-exported)
from .envs.spaces import Box
from .task_layers import _TaskLayer

NTERMS = len(SCHED_TERMS)
DONE_ROWS = {"reset": _abi.PERTURB_DONE_ROW_RESET, "terminal": _abi.PERTURB_DONE_ROW_TERMINAL}


# ---- the presets ----------------------------------------------------------------------------------------------------------------------------
def leg_pairs(hip_xy):
    """``(diagonals, laterals, fore_hind)`` -- three pairs of pairs of leg indices 0..3 -- from the four hips' ``(x, y)`` in the base
    frame (+x forward, +y left): legs on opposite sides and ends; on the same side; at the same end (fore pair first)."""
    hip_xy = np.asarray(hip_xy, np.float64)
    if hip_xy.shape != (4, 2) or (hip_xy == 0).any():
        raise ValueError(f"hip_xy: four (x, y) off both axes, got {hip_xy.tolist()}")
    fore, left = hip_xy[:, 0] > 0, hip_xy[:, 1] > 0
    legs = range(4)
    pick = lambda cond: tuple(i for i in legs if cond(i))
    pairs = (pick(lambda i: fore[i] == left[i]), pick(lambda i: fore[i] != left[i])), (pick(lambda i: left[i]), pick(lambda i: not left[i])), \
            (pick(lambda i: fore[i]), pick(lambda i: not fore[i]))
    if any(len(p) != 2 for kind in pairs for p in kind):
        raise ValueError(f"hip_xy: not one hip per quadrant: {hip_xy.tolist()}")
    return pairs


def gait_presets(hip_xy):
    """``{name: (offsets[4], duty)}``: ``trot`` (the diagonals alternate), ``pace`` (the sides alternate), ``bound`` (fore and hind pair
    alternate), ``pronk`` (all four together), each standing half a period; ``walk``, the four-beat lateral sequence hind-left,
    fore-left, hind-right, fore-right, standing three quarters."""
    diagonals, laterals, fore_hind = leg_pairs(hip_xy)
    hip_xy = np.asarray(hip_xy, np.float64)

    def two_beat(pair_a, pair_b):
        first = pair_a if 0 in pair_a else pair_b            # leg 0's pair leads
        return tuple(0.0 if i in first else 0.5 for i in range(4))

    order = sorted(range(4), key=lambda i: (hip_xy[i, 1] < 0, hip_xy[i, 0] > 0))       # left side first, hind before fore
    walk = [0.0] * 4
    for beat, i in enumerate(order):
        walk[i] = 0.25 * beat
    return {"trot": (two_beat(*diagonals), 0.5), "pace": (two_beat(*laterals), 0.5), "bound": (two_beat(*fore_hind), 0.5),
            "pronk": ((0.0, 0.0, 0.0, 0.0), 0.5), "walk": (tuple(walk), 0.75)}


def _packaged_hips():
    """The hips' ``(x, y)`` of the packaged robot: the femur bodies' positions in the FRAME (bodies 1, 4, 7, 10)."""
    with open(os.path.join(_abi.package_dir(), "model", "quadruped_model.json")) as fh:
        bodies = json.load(fh)["bodies"]
    return [bodies[1 + 3 * k]["pos"][:2] for k in range(4)]


GAITS = gait_presets(_packaged_hips())


term_weights = functools.partial(shaped.term_weights, terms=SCHED_TERMS)      # ``[4]`` floats in the order of ``SCHED_TERMS``


def gait_table(gaits) -> list:
    """``[(offsets[4], duty)]`` from preset names and / or ``(offsets, duty)`` rows; every value checked against the ABI's ranges."""
    rows = []
    if isinstance(gaits, str):
        gaits = (gaits,)
    for g in gaits:
        if isinstance(g, str):
            if g not in GAITS:
                raise ValueError(f"gaits: unknown preset {g!r}: one of {', '.join(GAITS)}")
            g = GAITS[g]
        offsets, duty = g
        offsets, duty = tuple(float(np.float32(o)) for o in offsets), float(np.float32(duty))
        if len(offsets) != 4 or not all(np.isfinite(o) and 0.0 <= o < 1.0 for o in offsets):
            raise ValueError(f"gaits: four offsets in [0, 1), got {offsets}")
        if not (np.isfinite(duty) and 1.0 / 64 <= duty <= 63.0 / 64):
            raise ValueError(f"gaits: duty in [1/64, 63/64], got {duty}")
        rows.append((offsets, duty))
    if not 1 <= len(rows) <= SCHED_MAX_GAITS:
        raise ValueError(f"gaits: 1 .. {SCHED_MAX_GAITS} rows, got {len(rows)}")
    return rows


class GaitSchedule(shaped.ShapedReward, _TaskLayer):
    """Bound to ``sensor`` (a ``ContactSensor``; this is its ``Handle`` child, so it is destroyed before it).  ``gaits``: preset names
    (``GAITS``) and / or ``(offsets[4], duty)`` rows, 1 to 8 of them; each episode of each env draws one of them, a frequency from
    ``freq = (lo, hi)`` Hz and, with ``random_phase``, its starting phase, keyed by ``(seed, env_index_base + i, episode)``.  The terms,
    the ramp ``kappa``, the stand gate and the treatment of finished envs (``done_row``: ``"terminal"`` where a finished env's row is
    its terminal observation, ``"reset"`` where it is the new episode's) are defined in ``include/quadgym.h``."""

    _destroy = "qg_sched_destroy"
    _abi_prefix = "qg_sched"
    TERMS = SCHED_TERMS
    DIM = SCHED_DIM
    COLUMNS = _abi.SCHED_COLUMNS

    def __init__(self, sensor, gaits=("trot",), freq=(1.5, 1.5), weights=None, random_phase: bool = False, done_row: str = "terminal",
                 kappa: float = 1.0 / 256, sigma_force: float = 5.0, sigma_velocity: float = 0.5, swing_height_target: float = 0.05,
                 min_command_speed: float = 0.1, seed: int = 0, env_index_base: int | None = None):
        w = term_weights(weights)
        table = gait_table(gaits)
        if done_row not in DONE_ROWS:
            raise ValueError(f"done_row must be 'reset' or 'terminal', got {done_row!r}")
        lo, hi = (float(np.float32(f)) for f in freq)
        if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= hi):
            raise ValueError(f"freq {tuple(freq)} must be finite with 0 < lo <= hi")
        limits = dict(kappa=kappa, sigma_force=sigma_force, sigma_velocity=sigma_velocity, swing_height_target=swing_height_target,
                      min_command_speed=min_command_speed)
        for name, value in limits.items():
            limits[name] = float(value)
            if not np.isfinite(limits[name]):
                raise ValueError(f"{name} must be finite, got {value}")
        if not 0.0 <= limits["kappa"] <= 1.0 / 128:
            raise ValueError(f"kappa must lie in 0 .. 1/128, got {kappa}")
        for name in ("sigma_force", "sigma_velocity"):
            if not limits[name] > 0.0:
                raise ValueError(f"{name} must be > 0, got {limits[name]}")
        if limits["min_command_speed"] < 0.0:
            raise ValueError(f"min_command_speed must be >= 0, got {min_command_speed}")
        super().__init__(sensor.device, parent=sensor)
        self.sensor, self.num_envs = sensor, sensor.num_envs
        self.weights = dict(zip(SCHED_TERMS, w))
        self.table, self.freq, self.done_row, self.random_phase = table, (lo, hi), done_row, bool(random_phase)
        for name, value in limits.items():
            setattr(self, name, value)
        base = getattr(getattr(sensor, "_parent", None), "env_index_base", 0) if env_index_base is None else env_index_base
        self.seed, self.env_index_base = int(seed), int(base)
        self.desc = QgSchedDesc.make(table, (lo, hi), w, random_phase, DONE_ROWS[done_row], seed=seed, env_index_base=self.env_index_base,
                                     **limits)
        self._create("qg_sched_create", sensor._h, C.byref(self.desc))

    def gaits(self):
        """NumPy (waits for the device): ``gait`` int32 ``[N]`` (the row of the table), ``freq`` float32 ``[N]`` and ``phi`` uint32
        ``[N]`` of the running episodes."""
        gait, freq, phi = np.empty(self.num_envs, np.int32), np.empty(self.num_envs, np.float32), np.empty(self.num_envs, np.uint32)
        check(self._lib.qg_sched_get_gaits(self._h, gait.ctypes.data, freq.ctypes.data, phi.ctypes.data), "qg_sched_get_gaits")
        return {"gait": gait, "freq": freq, "phi": phi}

    # -- device path ------------------------------------------------------------------------
    def _wide_pair(self, narrow, wide, names, width=None):
        """The checks of an ``(obs, out)`` pair: ``(obs pointer, obs stride, O, out pointer, out stride)``.  ``narrow`` may be None
        (``O = width or 0``) and may be ``wide[:, :O]`` itself (in place); any other overlap raises."""
        n_ptr, n_stride, O = None, 0, 0 if width is None else width
        if narrow is not None:
            if narrow.dim() != 2 or (width is not None and narrow.shape[1] != width):
                raise ValueError(f"{names[0]}: expected a float32 tensor of shape ({self.num_envs}, {'O' if width is None else width}), "
                                 f"got {tuple(narrow.shape)}")
            O = int(narrow.shape[1])
            n_stride, n_ptr = self._check_rows(narrow, O, names[0]), narrow.data_ptr()
        if wide is None:
            return n_ptr, n_stride, O, None, 0
        w_stride = self._check_rows(wide, O + SCHED_DIM, names[1])
        if narrow is not None:
            shaped.refuse_overlap(narrow, O, n_stride, wide, O + SCHED_DIM, w_stride,
                                  f"{names[0]} and {names[1]} overlap: allowed only where {names[0]} is {names[1]}[:, :O]")
        return n_ptr, n_stride, O, wide.data_ptr(), w_stride

    def step(self, done=None, reward=None, reward_out=None, components=None, base_components=None, command=None, obs=None, out=None,
             terminal_obs=None, terminal_out=None, stream=None):
        """One launch on ``stream`` (torch's current stream by default), behind the env-step whose state it is to see.  Returns
        ``(components, reward_out, out)``; ``components`` and ``reward_out`` are allocated unless passed, ``out`` (float32
        ``[N, O + 10]``, rows at a stride) only where ``obs`` (``[N, O]``) is given without it.

        ``done``, ``reward``, ``reward_out``, ``components``, ``base_components`` (``C0 <= 28`` columns) and ``command`` as
        ``GaitReward.step`` takes them; the command here makes the schedule say "stand" at or below ``min_command_speed``.  ``obs``
        may be ``out[:, :O]`` itself: only the ten columns are written.  ``terminal_obs`` / ``terminal_out`` likewise, with
        ``done_row="reset"`` only: the finished envs' rows get the old episode's columns.  A bad argument raises ``ValueError``
        before any launch."""
        import torch
        if terminal_out is not None and self.done_row != "reset":
            raise ValueError("terminal_out goes with done_row='reset': with 'terminal' the row itself is the terminal observation")
        if terminal_out is None and terminal_obs is not None:
            raise ValueError("terminal_obs without terminal_out")
        obs_ptr, obs_stride, O, out_ptr, out_stride = self._wide_pair(obs, out, ("obs", "out"))     # (out without obs: O = 0)
        t_ptr, t_stride, _, to_ptr, to_stride = self._wide_pair(terminal_obs, terminal_out, ("terminal_obs", "terminal_out"), O)
        if terminal_out is not None and terminal_obs is None and O:
            raise ValueError(f"terminal_out without terminal_obs: the rows in front are {O} wide")
        done3, rows11, components, reward_out = self._shaped_args(done, reward, reward_out, components, base_components, command)
        if obs is not None and out is None:
            out = torch.empty((self.num_envs, O + SCHED_DIM), device=self._torch_device(), dtype=torch.float32)
            out_ptr, out_stride = out.data_ptr(), O + SCHED_DIM
        check(self._lib.qg_sched_advance_device(self._h, *done3, *rows11, obs_ptr, obs_stride, O, out_ptr, out_stride, t_ptr, t_stride, to_ptr, to_stride,
                                           self._stream_ptr(stream)), "qg_sched_advance_device")
        return components, reward_out, out

    def begin(self, mask=None, rows=None, obs_dim: int | None = None, stream=None):
        """An explicit reset, one launch: the envs of ``mask`` (uint8 / bool ``[N]``, contiguous; None: all) start a new episode --
        its gait, frequency and starting phase --, and their rows of ``rows`` (float32 ``[N, O + 10]`` at a stride, optional) take the
        new episode's ten columns behind the ``O = obs_dim`` (default: the rows' width less 10) in front."""
        import torch
        m_ptr = r_ptr = None
        r_stride, O = 0, 0
        if mask is not None:
            if self._check_vec(mask, (torch.uint8, torch.bool), "mask") != 1:
                raise ValueError("mask must be contiguous")
            m_ptr = mask.data_ptr()
        if rows is not None:
            if rows.dim() != 2 or rows.shape[1] < SCHED_DIM:
                raise ValueError(f"rows: expected a float32 tensor of shape ({self.num_envs}, O + {SCHED_DIM}), got {tuple(rows.shape)}")
            O = int(rows.shape[1]) - SCHED_DIM if obs_dim is None else int(obs_dim)
            if not 0 <= O <= rows.shape[1] - SCHED_DIM:
                raise ValueError(f"obs_dim {obs_dim} outside 0 .. {rows.shape[1] - SCHED_DIM}")
            r_stride, r_ptr = self._check_rows(rows, int(rows.shape[1]), "rows"), rows.data_ptr()
        check(self._lib.qg_sched_begin_device(self._h, m_ptr, r_ptr, r_stride, O, self._stream_ptr(stream)), "qg_sched_begin_device")
        return rows


def clock_columns(table, gait, freq, phi):
    """The ten clock columns of ``(gait row, freq, phi)`` arrays in NumPy (float64 ``sin`` / ``cos``, rounded to float32): what the
    wrapper's cold path fills a reset row with where the device row holds the terminal observation."""
    gait, phi = np.asarray(gait, np.int64), np.asarray(phi, np.uint32)
    off = np.array([[np.uint32(int(np.rint(np.float64(np.float32(o)) * 2.0 ** 32)) % (1 << 32)) for o in offsets] for offsets, _ in table], np.uint32)
    D = np.array([int(np.rint(np.float64(np.float32(duty)) * 2.0 ** 32)) for _, duty in table], np.uint32)
    p = ((phi[:, None] + off[gait]) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    cols = np.concatenate([np.sin(2 * np.pi * p), np.cos(2 * np.pi * p), np.asarray(freq, np.float64)[:, None],
                           ((D[gait] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24)[:, None]], axis=1)
    return cols.astype(np.float32)


class DeviceGaitScheduleVecEnv(shaped.CommandGated, DeviceVecEnvWrapper):
    """The gait schedule around ``WalkingQuadrupedVecEnv`` or ``POWalkingQuadrupedVecEnv`` (or a device-side wrapper around one):
    ``obs_dim`` / ``observation_space`` / ``terminal_obs`` are 10 wider -- the clock columns behind the env's observation --,
    ``step_tensor`` runs the env's launch into the wrapper's own ``[N, O]`` rows, then the schedule's launch on the same stream, and
    ``reward`` comes back shaped.  ``components``, if passed, is ``[N, len(venv.reward_keys) + 4]``; ``reward_keys`` lists them, so
    ``RewardMonitor.for_env(wrapper)`` works as it is (around ``DeviceGaitRewardVecEnv``: 11 + 7 + 4 = 22 columns).  The sensor is the
    env's (``venv.contact_sensor(force_threshold)``); its timers are not touched.  ``reset()`` begins a new episode of the schedule;
    ``snapshot`` / ``restore`` carry the phases and episode counters.

    ``gate_on_command=True`` (the partially observable env only) makes the schedule say "stand" where the newest frame's command is at
    most ``min_command_speed`` in m/s: around a ``DeviceVecNormalize`` with ``norm_obs=True`` it is refused at construction (the order
    that works is ``DeviceVecNormalize(DeviceGaitScheduleVecEnv(env, gate_on_command=True))``).

    Stacking order: ``DevicePerturbedVecEnv`` goes INSIDE this wrapper (the clock is not a sensor: no noise on it; around this wrapper
    it is refused); ``DeviceGaitRewardVecEnv`` on either side; ``DevicePrivilegedVecEnv`` and ``DeviceVecNormalize`` OUTSIDE (a
    privileged pack inside would leave the clock out of the actor's window ``[0 : actor_obs_dim]``: refused).  The plain env has no
    command and steps into packed rows: it is refused, drive a ``GaitSchedule`` by hand there.  The NumPy ``reset()`` / ``step()``
    are a cold path built for correctness: they return wide rows, shaped rewards and leave ``last_schedule_components [N, 4]``.
    Every other attribute passes through to the wrapped env."""

    _snapshot_key = "gait_schedule"

    def __init__(self, venv, gaits=("trot",), freq=(1.5, 1.5), weights=None, force_threshold: float = 1.0, gate_on_command: bool = False,
                 seed: int = 0, env_index_base: int | None = None, **options):
        if venv.packed_step:
            raise ValueError("DeviceGaitScheduleVecEnv around the plain env: its packed step has no command and no room for the clock "
                             "columns; wrap WalkingQuadrupedVecEnv or POWalkingQuadrupedVecEnv, or drive a GaitSchedule by hand: "
                             "GaitSchedule(env.contact_sensor(threshold)).step(...) behind env.step_tensor(...)")
        if stack_layer(venv, "privileged") is not None:
            raise ValueError("DeviceGaitScheduleVecEnv around DevicePrivilegedVecEnv: the actor's window [0 : actor_obs_dim] would miss the "
                             "clock columns; put the schedule inside, DevicePrivilegedVecEnv(DeviceGaitScheduleVecEnv(env))")
        self._check_gate(venv, gate_on_command,
                         "put the schedule inside, DeviceVecNormalize(DeviceGaitScheduleVecEnv(env, gate_on_command=True))")
        po = hasattr(venv, "obs_window")                    # its finished rows hold the new episode's reset stack
        base = venv._sim.env_index_base if env_index_base is None else env_index_base
        self.schedule = GaitSchedule(venv.contact_sensor(force_threshold), gaits, freq, weights, done_row="reset" if po else "terminal",
                                     seed=seed, env_index_base=base, **options)
        super().__init__(venv, self.schedule)
        self.gate_on_command = bool(gate_on_command)
        self.inner_obs_dim = int(venv.obs_dim)
        self.obs_dim = self.inner_obs_dim + SCHED_DIM
        self.observation_space = Box(low=-np.inf, high=np.inf, shape=(self.obs_dim,), dtype=np.float32)
        self.last_schedule_components = None
        self._narrow = self._narrow_term = self._base = None          # the env's own rows of a step_tensor call

    @property
    def reward_keys(self):
        return list(self.venv.reward_keys) + list(SCHED_TERMS)

    # -- device path ------------------------------------------------------------------------
    def step_tensor(self, actions, *args, **kwargs):
        """The wrapped env's ``step_tensor`` with its signature: ``obs`` (and ``terminal_obs``, where the env takes it) is
        ``[N, O + 10]``, ``reward`` comes back shaped in place and ``components``, if passed, is ``[N, len(reward_keys)]``."""
        stream = kwargs.get("stream")
        O, sched = self.inner_obs_dim, self.schedule
        bound = self._step_buffers(args, kwargs)
        if "obs" not in bound:
            raise ValueError("step_tensor: obs is required")
        wide, wide_term, comps = bound["obs"], bound.get("terminal_obs"), bound.get("components")
        sched._check_rows(wide, self.obs_dim, "obs")                    # before the env's launch, every one of them
        if wide_term is not None:
            if sched.done_row != "reset":
                raise ValueError("terminal_obs: this env's step_tensor takes none (a finished env's row is its terminal observation)")
            sched._check_rows(wide_term, self.obs_dim, "terminal_obs")
        c0 = len(self.venv.reward_keys)
        if comps is not None:
            sched._check_rows(comps, c0 + NTERMS, "components")
        inner = dict(zip(STEP_BUFFERS, args), **kwargs)           # the positional buffers by name
        inner["obs"] = self._rows("_narrow", O)                   # the env writes contiguous rows; the schedule's launch copies them in front
        if wide_term is not None:
            inner["terminal_obs"] = self._rows("_narrow_term", O)
        if comps is not None:
            inner["components"] = self._rows("_base", c0)
        self.venv.step_tensor(actions, **inner)
        sched.step(bound["done"], bound["reward"], bound["reward"], comps, inner.get("components") if comps is not None else None,
                   self._command(inner["obs"]), inner["obs"], wide, inner.get("terminal_obs") if wide_term is not None else None, wide_term,
                   stream=stream)
        return None

    # -- NumPy cold path --------------------------------------------------------------------
    def _wide(self, obs):
        import torch
        wide = torch.zeros((self.num_envs, self.obs_dim), device=self.schedule._torch_device(), dtype=torch.float32)
        wide[:, :self.inner_obs_dim] = self._upload(obs)
        return wide

    def reset(self):
        self.last_schedule_components = None
        return self.schedule.begin(rows=self._wide(self.venv.reset())).cpu().numpy()

    def step_async(self, actions):
        self.venv.step_async(actions)

    def step_wait(self):
        """The host envs return a finished env's reset observation in ``obs`` and its last one in ``infos``.  Where the device row is
        the reset stack (``done_row="reset"``) the terminal rows travel beside it as ``terminal_obs``; where it is the terminal
        observation, that goes through the launch in the row's place and the reset row's clock columns are formed on the host from
        the new episode's draws (``clock_columns``)."""
        obs, rew, done, infos = self.venv.step_wait()
        sched, O = self.schedule, self.inner_obs_dim
        obs = np.array(obs, dtype=np.float32)
        finished = [i for i, _ in self._finished_with_terminal(done, infos)]
        reset_rows = sched.done_row == "reset"
        term = np.zeros_like(obs)
        for i in finished:
            term[i] = infos[i]["terminal_observation"]
        rows = obs.copy()
        if not reset_rows:
            rows[finished] = term[finished]
        wide = self._wide(rows)
        wide_term = self._wide(term) if reset_rows and finished else None
        command = self._command(wide[:, :O]) if self.gate_on_command else None
        comps, shaped, _ = sched.step(self._upload(done, np.uint8), self._upload(rew), command=command, obs=wide[:, :O], out=wide,
                                      terminal_obs=None if wide_term is None else wide_term[:, :O], terminal_out=wide_term)
        self.last_schedule_components = comps.cpu().numpy()
        out = wide.cpu().numpy()
        term_rows = wide_term.cpu().numpy() if wide_term is not None else out.copy()
        if not reset_rows and finished:
            now = sched.gaits()
            out[finished, :O] = obs[finished]
            out[finished, O:] = clock_columns(sched.table, now["gait"], now["freq"], now["phi"])[finished]
        for i in finished:
            info = dict(infos[i])
            info["terminal_observation"] = term_rows[i].copy()
            infos[i] = info
        return out, shaped.cpu().numpy(), done, infos

    # -- checkpoint / resume ----------------------------------------------------------------
    def _layer_state(self):
        return self.schedule.state()

    def _load_layer_state(self, state):
        self.schedule.load_state(state)
