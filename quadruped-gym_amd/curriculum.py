"""``CommandCurriculum`` and ``DeviceCommandCurriculumVecEnv`` -- a curriculum over the commanded (speed, velocity angle) that stays on
the GPU (``qg_cmdcur_*`` of ``include/quadgym.h``, ``csrc/qg_cmdcur.hip``): a grid of bins with integer weights that grow outward from
an easy region as the segments drawn from a bin succeed (Margolis et al., "Rapid Locomotion via Reinforcement Learning", in exact
integers), optional resampling inside an episode, and the commands in force as a device tensor.

Two launches of hand-written gfx950 code behind the env-step; they write the walking layer's command slots, so the step kernels are
the ones every other env runs.  PyTorch is plumbing only; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import CMDCUR_MAX_CRITERIA, CMDCUR_MAX_SIDE, CMDCUR_MAX_WEIGHT, QgCmdCurDesc, check
from ._abi import CMDCUR_MAX_BINS, QgCmdCurCriterion                           # (re-exported: names this module has always had)
from .envs.device_wrapper import STEP_BUFFERS, DeviceVecEnvWrapper, base_env, stack_layers
from .task_layers import _TaskLayer


def grid_edges(speed, bins):
    """``(speed_edges [n_speed + 1], alpha_edges [n_alpha + 1])`` in float32, formed as the ABI forms them: the widths in float64
    rounded once, every edge one float32 product and one float32 add."""
    lo, hi = np.float32(speed[0]), np.float32(speed[1])
    ns, na = int(bins[0]), int(bins[1])
    ws = np.float32((np.float64(hi) - np.float64(lo)) / ns)
    wa = np.float32(2.0 * np.pi / na)
    s = lo + np.arange(ns + 1, dtype=np.float32) * ws
    a = np.float32(-np.pi) + np.arange(na + 1, dtype=np.float32) * wa
    return s.astype(np.float32), a.astype(np.float32)


def check_weights(weights, n_bins, weight_max, what="weights"):
    """``weights`` as int32 ``[n_bins]`` within ``0 .. weight_max`` with at least one above 0, or ``ValueError``."""
    w = np.asarray(weights)
    if w.shape != (n_bins,) or not np.issubdtype(w.dtype, np.integer):
        raise ValueError(f"{what}: expected {n_bins} integers, got {w.dtype} {w.shape}")
    if (w < 0).any() or (w > weight_max).any() or not (w > 0).any():
        raise ValueError(f"{what}: every weight in 0 .. {weight_max} and at least one above 0")
    return np.ascontiguousarray(w, dtype=np.int32)


class CommandCurriculum(_TaskLayer):
    """Bound to ``walk`` (a ``WalkLayer``; this is its ``Handle`` child, so it is destroyed before it).  ``speed = (lo, hi)`` and
    ``bins = (n_speed, n_alpha)`` span the grid; ``initial_weights`` (``[n_speed * n_alpha]`` integers in ``0 .. weight_max``) say
    where it starts; a successful segment adds ``delta`` to its bin and the bin's neighbours.  A segment ends with its episode and,
    with ``resample_steps = R > 0``, after ``R`` env-steps; it succeeds where it lasted ``min_steps`` and every criterion
    ``(column, sense, threshold)`` holds on the mean per step of that column of the step's components.  The formulas, roundings and
    orders are ``include/quadgym.h``'s."""

    _destroy = "qg_cmdcur_destroy"
    _abi_prefix = "qg_cmdcur"

    def __init__(self, walk, speed=(0.0, 1.0), bins=(4, 4), initial_weights=None, weight_max: int = 64, delta: int = 8,
                 resample_steps: int = 0, min_steps: int = 1, criteria=(), fixed_heading: float | None = None, seed: int = 0,
                 env_index_base: int | None = None):
        ns, na = (int(b) for b in bins)
        if not (1 <= ns <= CMDCUR_MAX_SIDE and 1 <= na <= CMDCUR_MAX_SIDE):
            raise ValueError(f"bins {tuple(bins)}: each side 1 .. {CMDCUR_MAX_SIDE}")
        lo, hi = (float(np.float32(s)) for s in speed)
        if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
            raise ValueError(f"speed {tuple(speed)} must be finite with lo <= hi")
        if not 1 <= int(weight_max) <= CMDCUR_MAX_WEIGHT:
            raise ValueError(f"weight_max must lie in 1 .. {CMDCUR_MAX_WEIGHT}, got {weight_max}")
        if not 1 <= int(delta) <= int(weight_max):
            raise ValueError(f"delta must lie in 1 .. weight_max = {weight_max}, got {delta}")
        if int(resample_steps) < 0:
            raise ValueError(f"resample_steps must be >= 0, got {resample_steps}")
        if int(min_steps) < 1:
            raise ValueError(f"min_steps must be >= 1, got {min_steps}")
        if fixed_heading is not None and not np.isfinite(float(fixed_heading)):
            raise ValueError(f"fixed_heading must be finite, got {fixed_heading}")
        criteria = [(int(c), int(s), float(t)) for c, s, t in criteria]
        if len(criteria) > CMDCUR_MAX_CRITERIA:
            raise ValueError(f"criteria: at most {CMDCUR_MAX_CRITERIA}, got {len(criteria)}")
        for c, s, t in criteria:
            if c < 0 or s not in (1, -1) or not np.isfinite(t):
                raise ValueError(f"criteria: (column >= 0, sense +1 or -1, finite threshold), got {(c, s, t)}")
        if initial_weights is None:
            initial_weights = np.full(ns * na, int(weight_max), np.int32)
        w = check_weights(initial_weights, ns * na, int(weight_max), "initial_weights")
        super().__init__(walk.device, parent=walk)
        self.walk, self.num_envs = walk, walk.num_envs
        self.speed, self.shape, self.n_bins = (lo, hi), (ns, na), ns * na
        self.weight_max, self.delta, self.resample_steps, self.min_steps = int(weight_max), int(delta), int(resample_steps), int(min_steps)
        self.criteria, self.fixed_heading = criteria, None if fixed_heading is None else float(np.float32(fixed_heading))
        base = getattr(getattr(walk, "_parent", None), "env_index_base", 0) if env_index_base is None else env_index_base
        self.seed, self.env_index_base = int(seed), int(base)
        self.desc = QgCmdCurDesc.make((lo, hi), (ns, na), w.tolist(), weight_max, delta, resample_steps, min_steps, criteria, fixed_heading,
                                      seed, self.env_index_base)
        self._create("qg_cmdcur_create", walk._h, C.byref(self.desc))

    def grid(self):
        """``(speed_edges, alpha_edges)`` float32: bin ``(si, ai)`` draws from ``[speed_edges[si], speed_edges[si] + ws)`` and
        ``[alpha_edges[ai], alpha_edges[ai] + wa)``."""
        return grid_edges(self.speed, self.shape)

    def weights(self):
        """NumPy int32 ``[n_speed, n_alpha]`` (waits for the device): the current weights."""
        w = np.empty(self.n_bins, np.int32)
        check(self._lib.qg_cmdcur_get_weights(self._h, w.ctypes.data), "qg_cmdcur_get_weights")
        return w.reshape(self.shape)

    def set_weights(self, weights):
        """Replaces the current weights (``[n_speed, n_alpha]`` or flat integers, validated as the initial ones): how a multi-rank
        trainer merges its shards' grids."""
        w = check_weights(np.asarray(weights).reshape(-1), self.n_bins, self.weight_max)
        check(self._lib.qg_cmdcur_set_weights(self._h, w.ctypes.data), "qg_cmdcur_set_weights")

    def stats(self):
        """NumPy int64 ``[n_speed, n_alpha]`` each: ``episodes`` (judged segments) and ``successes`` per bin."""
        ep, su = np.empty(self.n_bins, np.int64), np.empty(self.n_bins, np.int64)
        check(self._lib.qg_cmdcur_get_stats(self._h, ep.ctypes.data, su.ctypes.data), "qg_cmdcur_get_stats")
        return {"episodes": ep.reshape(self.shape), "successes": su.reshape(self.shape)}

    def bins(self):
        """NumPy (waits for the device): ``bin`` int32 ``[N]``, ``steps`` int32 ``[N]`` and ``segment`` int64 ``[N]`` of the running
        segments."""
        bin_, steps, seg = np.empty(self.num_envs, np.int32), np.empty(self.num_envs, np.int32), np.empty(self.num_envs, np.int64)
        check(self._lib.qg_cmdcur_get_bins(self._h, bin_.ctypes.data, steps.ctypes.data, seg.ctypes.data), "qg_cmdcur_get_bins")
        return {"bin": bin_, "steps": steps, "segment": seg}

    # -- device path ------------------------------------------------------------------------
    def step(self, done, components, command_out=None, stream=None):
        """The two launches on ``stream`` (torch's current stream by default), behind the env-step whose ``done`` (uint8, bool or
        float32 ``[N]``, or None) and ``components`` (float32 ``[N, C]`` rows at a stride; None only without criteria) they read.
        ``command_out`` (float32 ``[N, 4]`` rows at a stride, optional) receives ``(vx, vy, hx, hy)`` of every env after the launch.
        A bad argument raises ``ValueError`` before any launch.  Returns ``command_out``."""
        d_ptr, kind, d_stride = self._done_arg(done)
        c_ptr, c_stride, n_columns = None, 0, 0
        if components is None:
            if self.criteria:
                raise ValueError(f"components: required, the curriculum has {len(self.criteria)} criteria")
        else:
            if components.dim() != 2:
                raise ValueError(f"components: expected a float32 tensor of shape ({self.num_envs}, C), got {tuple(components.shape)}")
            n_columns = int(components.shape[1])
            c_stride, c_ptr = self._check_rows(components, n_columns, "components"), components.data_ptr()
        for column, _, _ in self.criteria:
            if column >= n_columns:
                raise ValueError(f"components: {n_columns} columns, a criterion reads column {column}")
        o_ptr, o_stride = None, 4
        if command_out is not None:
            o_stride, o_ptr = self._check_rows(command_out, 4, "command_out"), command_out.data_ptr()
        check(self._lib.qg_cmdcur_advance_device(self._h, d_ptr, kind, d_stride, c_ptr, c_stride, n_columns, o_ptr, o_stride,
                                                 self._stream_ptr(stream)), "qg_cmdcur_advance_device")
        return command_out

    def begin(self, mask=None, stream=None):
        """An explicit reset, one launch: the envs of ``mask`` (uint8 / bool ``[N]``, contiguous; None: all) drop their running
        segment unjudged and draw a new one from the weights as they stand."""
        import torch
        m_ptr = None
        if mask is not None:
            if self._check_vec(mask, (torch.uint8, torch.bool), "mask") != 1:
                raise ValueError("mask must be contiguous")
            m_ptr = mask.data_ptr()
        check(self._lib.qg_cmdcur_begin_device(self._h, m_ptr, self._stream_ptr(stream)), "qg_cmdcur_begin_device")


def initial_weights_for(speed, bins, initial_speed, weight_max):
    """int32 ``[n_speed * n_alpha]``: ``weight_max`` for the bins whose speed interval ``[edge, next edge]`` meets
    ``initial_speed = (lo, hi)``, 0 for the others; ``ValueError`` where none does."""
    edges, _ = grid_edges(speed, bins)
    lo, hi = np.float32(initial_speed[0]), np.float32(initial_speed[1])
    if not lo <= hi:
        raise ValueError(f"initial_speed {tuple(initial_speed)}: lo <= hi")
    meets = (edges[:-1] <= hi) & (edges[1:] >= lo)
    if not meets.any():
        raise ValueError(f"initial_speed {tuple(initial_speed)} meets no bin of the speed range {tuple(speed)}")
    return np.repeat(np.where(meets, int(weight_max), 0).astype(np.int32), int(bins[1]))


class DeviceCommandCurriculumVecEnv(DeviceVecEnvWrapper):
    """The command curriculum around ``WalkingQuadrupedVecEnv`` or ``POWalkingQuadrupedVecEnv`` (or a device-side wrapper around one).
    ``step_tensor`` runs the stack's launches, then the curriculum's two on the same stream; observations, rewards and components pass
    through untouched, and the env-step that follows rewards (and shows, in a partially observable frame) the commands the curriculum
    wrote.  The reset row a partially observable step writes for a finished env shows the command of the segment that finished, as in
    the reference and with the in-kernel sampler.  ``criteria = {reward_key: (sense, threshold)}`` names columns of the wrapped
    stack's ``reward_keys``; the bins whose speed interval meets ``initial_speed`` start at ``weight_max``, the others at 0.
    ``commands_tensor`` (float32 ``[N, 4]``: vx, vy, hx, hy) holds the commands in force after the latest step, reset or restore.

    Refused at construction, before any handle exists: the plain env (no walking layer, no command) and an env with
    ``random_controls=True`` (its host sampler, or its in-kernel one, would redraw what the curriculum draws).  The wrapper touches no
    row, reward or component, so no order is refused: it goes on either side of ``DeviceVecNormalize``, ``DevicePerturbedVecEnv``,
    ``DeviceGaitRewardVecEnv``, ``DeviceGaitScheduleVecEnv`` and ``DevicePrivilegedVecEnv``; criteria on gait or schedule terms need it
    outside the wrapper that writes those columns (``envs/device_wrapper.py`` has the orders the suite steps).
    ``reset()`` begins a new segment for every env; ``snapshot`` / ``restore`` carry the grid and the segments.  The NumPy
    ``reset()`` / ``step()`` are a cold path built for correctness.  Every other attribute passes through to the wrapped env."""

    _snapshot_key = "command_curriculum"

    def __init__(self, venv, speed=(0.0, 1.0), bins=(4, 4), initial_speed=None, criteria=None, weight_max: int = 64, delta: int = 8,
                 resample_steps: int = 0, min_steps: int = 1, fixed_heading: float | None = None, seed: int = 0,
                 env_index_base: int | None = None):
        env = base_env(venv)
        if venv.packed_step or not hasattr(env, "_walk"):
            raise ValueError("DeviceCommandCurriculumVecEnv around the plain env: it has no walking layer and no command; wrap "
                             "WalkingQuadrupedVecEnv or POWalkingQuadrupedVecEnv")
        if getattr(env, "random_controls", False):
            raise ValueError("DeviceCommandCurriculumVecEnv around an env with random_controls=True: its own sampler would redraw the "
                             "commands the curriculum draws; build the env with random_controls=False")
        keys = list(venv.reward_keys)
        unknown = sorted(set(criteria or {}) - set(keys))
        if unknown:
            raise ValueError(f"criteria: unknown reward keys {unknown}: one of {', '.join(keys)}")
        rows = [(keys.index(key), int(sense), float(threshold)) for key, (sense, threshold) in (criteria or {}).items()]
        initial = initial_weights_for(speed, bins, speed if initial_speed is None else initial_speed, weight_max)
        base = env._sim.env_index_base if env_index_base is None else env_index_base
        self.curriculum = CommandCurriculum(env._walk, speed, bins, initial, weight_max, delta, resample_steps, min_steps, rows, fixed_heading,
                                            seed, base)
        super().__init__(venv, self.curriculum)
        self.criteria = dict(criteria or {})
        self._columns = len(keys)
        self._comps = None                   # the stack's component columns of a step_tensor call that passed none
        self.commands_tensor = None
        self._refresh_commands()

    def _refresh_commands(self):
        """``commands_tensor`` from the walking layer's slots (waits for the device): what no advance has written yet."""
        import torch
        velocity, heading = base_env(self.venv).commands()
        host = np.concatenate([velocity, heading], axis=1).astype(np.float32)
        if self.commands_tensor is None:
            self.commands_tensor = torch.empty((self.num_envs, 4), device=self.curriculum._torch_device(), dtype=torch.float32)
        self.commands_tensor.copy_(torch.from_numpy(host))

    # -- device path ------------------------------------------------------------------------
    def step_tensor(self, actions, *args, **kwargs):
        """The wrapped env's ``step_tensor`` with its signature, then the curriculum's launches on the same stream."""
        import torch
        stream = kwargs.get("stream")
        bound = self._step_buffers(args, kwargs)
        comps = bound.get("components")
        if comps is None and self.criteria:
            if self._comps is None:
                self._comps = torch.empty((self.num_envs, self._columns), device=self.curriculum._torch_device(), dtype=torch.float32)
            comps = self._comps
            kwargs = dict(zip(STEP_BUFFERS, args), **kwargs)
            kwargs["components"], args = comps, ()
        if comps is not None:
            self.curriculum._check_rows(comps, self._columns, "components")       # before the env's launch
        self.venv.step_tensor(actions, *args, **kwargs)
        self.curriculum.step(bound["done"], comps, self.commands_tensor, stream=stream)
        return None

    # -- NumPy cold path --------------------------------------------------------------------
    def _host_components(self):
        """The latest step's component columns of the whole wrapped stack, ``[N, len(venv.reward_keys)]``."""
        cols = [np.asarray(base_env(self.venv).last_components, np.float32)]
        for layer in reversed(list(stack_layers(self.venv))):
            for name in ("last_gait_components", "last_schedule_components"):
                if name in vars(layer):
                    cols.append(np.asarray(getattr(layer, name), np.float32))
        return np.concatenate(cols, axis=1)

    def reset(self):
        obs = self.venv.reset()
        self.curriculum.begin()
        self._refresh_commands()
        return obs

    def step_async(self, actions):
        self.venv.step_async(actions)

    def step_wait(self):
        obs, rew, done, infos = self.venv.step_wait()
        comps = self._upload(self._host_components()) if self.criteria else None
        self.curriculum.step(self._upload(done, np.uint8), comps, self.commands_tensor)
        return obs, rew, done, infos

    # -- checkpoint / resume ----------------------------------------------------------------
    def _layer_state(self):
        return self.curriculum.state()

    def _load_layer_state(self, state):
        self.curriculum.load_state(state)

    def restore(self, snap):
        super().restore(snap)
        self._refresh_commands()
