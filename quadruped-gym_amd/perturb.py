"""``Perturbation`` and ``DevicePerturbedVecEnv`` -- sensor noise, a per-episode sensor bias and actuation latency on rows that stay
on the GPU (``qg_perturb_*`` of ``include/quadgym.h``, ``csrc/qg_perturb.hip``).

An env-step costs two small launches of hand-written gfx950 code on the caller's stream: one between the policy and the env (the
action ring, the delayed row, action noise), one behind the env (observation noise and bias per frame column).  Every draw is keyed
by (seed, global env index, episode, frame, column): shards reproduce one big handle, a replayed hipGraph draws fresh noise, and a
frame keeps its noise while it moves through an ``obs_window`` stack.  PyTorch is plumbing only; there is no CPU path.

Not modelled: noise ahead of the Madgwick filter (the ``euler`` columns take independent noise of their own), latency shorter than
an env-step, observation latency, a random-walk bias, noise on rewards.  The partially observable frame's ``data.ctrl`` columns show
what the servos received -- the delayed action -- and are left as the env wrote them.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import QgPerturbDesc, check
from ._handle import Handle
from .envs.device_wrapper import DeviceVecEnvWrapper, stack_layer

# frame columns by name, per layout (width -> {group: slice}): the partially observable frame (po_walking_quad.py:48-56) and the
# 33- and 21-value sensor packs (QG_OBS_FULL, QG_OBS_IMU)
COLUMN_GROUPS = {
    26: {"gyro": slice(0, 3), "accel": slice(3, 6), "euler": slice(6, 9), "body_vel": slice(9, 11), "ctrl": slice(11, 23),
         "command": slice(23, 26)},
    33: {"jointpos": slice(0, 12), "accel": slice(12, 15), "gyro": slice(15, 18), "pos": slice(18, 21), "linvel": slice(21, 24),
         "xaxis": slice(24, 27), "zaxis": slice(27, 30), "body_vel": slice(30, 33)},
    21: {"jointpos": slice(0, 12), "accel": slice(12, 15), "gyro": slice(15, 18), "body_vel": slice(18, 21)},
}


def column_stds(spec, frame_dim: int):
    """``[frame_dim]`` float32 from None (zeros), a scalar (every column), a sequence of ``frame_dim`` values, or a dict of column
    groups by name (``COLUMN_GROUPS[frame_dim]``; a value is a scalar or one number per column of the group)."""
    out = np.zeros(int(frame_dim), np.float32)
    if spec is None:
        return out
    if isinstance(spec, dict):
        groups = COLUMN_GROUPS.get(int(frame_dim))
        if groups is None:
            raise ValueError(f"no named columns for frames of {frame_dim} values: pass a sequence")
        for name, val in spec.items():
            if name not in groups:
                raise ValueError(f"column group {name!r}: one of {sorted(groups)}")
            out[groups[name]] = val
        return out
    out[:] = spec                                            # a scalar, or frame_dim values (anything else raises)
    return out


class Perturbation(Handle):
    """The perturbation layer of ``include/quadgym.h``: ``perturb_actions`` before the env, ``observe`` (or ``observe_packed``)
    behind it, ``begin`` for an explicit reset.  ``delays`` are env-steps ``(lo, hi)``; ``max_delay`` (the ring's depth) defaults to
    ``hi``.  ``done_row`` says what a finished env's row holds: ``"reset"`` (the partially observable env) or ``"terminal"``."""

    _destroy = "qg_perturb_destroy"
    _DONE_ROWS = {"reset": _abi.PERTURB_DONE_ROW_RESET, "terminal": _abi.PERTURB_DONE_ROW_TERMINAL}

    def __init__(self, num_envs: int, frame_dim: int, window: int = 1, obs_std=None, bias_std=None, action_std: float = 0.0,
                 delays=(0, 0), max_delay: int | None = None, reset_action=None, done_row: str = "terminal", seed: int = 0,
                 env_index_base: int = 0, device: int = 0):
        super().__init__(device)
        if done_row not in self._DONE_ROWS:
            raise ValueError("done_row must be 'reset' or 'terminal'")
        self.num_envs, self.frame_dim, self.window = int(num_envs), int(frame_dim), int(window)
        self.obs_dim = self.frame_dim * self.window          # the row width `_check_obs` asks for
        self.delay_range = (int(delays[0]), int(delays[1]))
        self.max_delay = self.delay_range[1] if max_delay is None else int(max_delay)
        self.done_row = done_row
        self.desc = QgPerturbDesc.make(self.num_envs, self.frame_dim, self.window, self.max_delay, self.delay_range, action_std,
                                       column_stds(obs_std, frame_dim), column_stds(bias_std, frame_dim), reset_action,
                                       self._DONE_ROWS[done_row], seed, env_index_base)
        self._create("qg_perturb_create", self.device, C.byref(self.desc))

    # -- device path ------------------------------------------------------------------------
    def perturb_actions(self, actions, out=None, stream=None):
        """``actions`` float32 ``[N, 12]``: the ring takes it, ``out`` (default: in place) gets what the servos receive."""
        import torch
        self._check_tensor(actions, (self.num_envs, _abi.NU), torch.float32, "actions")
        out = actions if out is None else out
        self._check_tensor(out, (self.num_envs, _abi.NU), torch.float32, "out")
        check(self._lib.qg_perturb_actions_device(self._h, self.num_envs, actions.data_ptr(), out.data_ptr(), self._stream_ptr(stream)),
              "qg_perturb_actions_device")
        return out

    def observe(self, obs, done=None, terminal_obs=None, out=None, stream=None):
        """``obs`` float32 ``[N, window * frame_dim]`` (strided rows allowed) as the env left it, ``done`` uint8 / bool / float32
        ``[N]`` at any stride or None, ``terminal_obs`` (``done_row="reset"`` only) perturbed in place.  ``out`` defaults to in
        place.  Advances every env's age, and the episode of those that finished.  Returns ``out``."""
        _, in_stride = self._check_obs(obs, self.num_envs)
        out = obs if out is None else out
        _, out_stride = self._check_obs(out, self.num_envs, "out")
        t_ptr, t_stride = None, 0
        if terminal_obs is not None:
            _, t_stride = self._check_obs(terminal_obs, self.num_envs, "terminal_obs")
            t_ptr = terminal_obs.data_ptr()
        d_ptr, kind, d_stride = self._done_arg(done)
        check(self._lib.qg_perturb_observe_device(self._h, self.num_envs, obs.data_ptr(), in_stride, out.data_ptr(), out_stride, t_ptr,
                                                  t_stride, d_ptr, kind, d_stride, self._stream_ptr(stream)), "qg_perturb_observe_device")
        return out

    def observe_packed(self, packed, stream=None):
        """The plain env's packed rows ``[N, obs_dim + 2]`` (obs, reward, done as float32) in place; reward and done are not touched."""
        D = self.obs_dim
        self._check_packed(packed, "packed")
        self.observe(packed[:, :D], packed[:, D + 1], stream=stream)
        return packed

    def begin(self, mask=None, rows=None, stream=None):
        """An explicit reset: the envs of ``mask`` (uint8 / bool ``[N]``, contiguous; None: all) start a new episode, and their rows of
        ``rows`` (the reset observations, optional) take frame-0 noise in place."""
        import torch
        m_ptr = r_ptr = None
        r_stride = 0
        if mask is not None:
            if self._check_vec(mask, (torch.uint8, torch.bool), "mask") != 1:
                raise ValueError("mask must be contiguous")
            m_ptr = mask.data_ptr()
        if rows is not None:
            _, r_stride = self._check_obs(rows, self.num_envs, "rows")
            r_ptr = rows.data_ptr()
        check(self._lib.qg_perturb_begin_device(self._h, self.num_envs, m_ptr, r_ptr, r_stride, self._stream_ptr(stream)),
              "qg_perturb_begin_device")
        return rows

    # -- state ------------------------------------------------------------------------------
    def delays(self):
        """``[N]`` int32: each env's delay in env-steps for its running episode (waits for the device)."""
        d = np.empty(self.num_envs, np.int32)
        check(self._lib.qg_perturb_get_delays(self._h, d.ctypes.data), "qg_perturb_get_delays")
        return d

    def state(self):
        """NumPy (waits for the device): ``age`` int32 ``[N]``, ``episode`` int64 ``[N]``, ``ring`` float32 ``[max_delay + 1, N, 12]``."""
        age, episode = np.empty(self.num_envs, np.int32), np.empty(self.num_envs, np.int64)
        ring = np.empty((self.max_delay + 1, self.num_envs, _abi.NU), np.float32)
        check(self._lib.qg_perturb_get_state(self._h, age.ctypes.data, episode.ctypes.data, ring.ctypes.data), "qg_perturb_get_state")
        return {"age": age, "episode": episode, "ring": ring}

    def load_state(self, state):
        age = np.ascontiguousarray(state["age"], dtype=np.int32)
        episode = np.ascontiguousarray(state["episode"], dtype=np.int64)
        ring = np.ascontiguousarray(state["ring"], dtype=np.float32)
        if age.shape != (self.num_envs,) or episode.shape != (self.num_envs,) or ring.shape != (self.max_delay + 1, self.num_envs, _abi.NU):
            raise ValueError(f"the state was taken from a layer of another shape: age {age.shape}, episode {episode.shape}, ring {ring.shape}")
        check(self._lib.qg_perturb_set_state(self._h, age.ctypes.data, episode.ctypes.data, ring.ctypes.data), "qg_perturb_set_state")


class DevicePerturbedVecEnv(DeviceVecEnvWrapper):
    """Sensor noise, sensor bias and actuation latency around ``QuadrupedVecEnv``, ``WalkingQuadrupedVecEnv`` or
    ``POWalkingQuadrupedVecEnv``; ``step_tensor`` stays on the device: ``perturb_actions``, the env's launch with the delayed actions,
    ``observe``, all on one stream.  ``obs_noise`` / ``obs_bias``: standard deviations per frame column -- a scalar, a sequence, or a
    dict by column group (``COLUMN_GROUPS``: ``gyro``, ``accel``, ``euler``, ``body_vel`` of the partially observable frame; the
    sensor groups of the 33- and 21-value packs).  ``action_latency = (lo, hi)`` in seconds, converted with timestep x frame_skip
    (rounded to nearest) as ``push_randomization`` converts.  The caller's ``actions`` tensor is left as the policy wrote it (it is
    what a rollout buffer stores).  The NumPy ``reset()`` / ``step()`` are a cold path built for correctness only.  Every other
    attribute passes through to the wrapped env.

    Stacking order: next to the env.  Around a stack that holds ``DevicePrivilegedVecEnv`` it is refused at construction, before any
    handle exists (the noise would land on the truth columns, or meet rows of another width after the launch): the order that works
    is ``DevicePrivilegedVecEnv(DevicePerturbedVecEnv(env))``."""

    _snapshot_key = "perturbation"

    def __init__(self, venv, obs_noise=None, obs_bias=None, action_noise: float = 0.0, action_latency=(0.0, 0.0), seed: int = 0,
                 env_index_base: int | None = None, device: int | None = None):
        import torch
        if stack_layer(venv, "privileged") is not None:     # before any handle: the noise would land on the truth columns
            raise ValueError("DevicePerturbedVecEnv around DevicePrivilegedVecEnv: sensor noise, bias and latency belong on the actor's "
                             "columns only; put it inside, DevicePrivilegedVecEnv(DevicePerturbedVecEnv(env))")
        if stack_layer(venv, "gait_schedule") is not None:  # the clock columns are no sensor, and the rows are no whole frames any more
            raise ValueError("DevicePerturbedVecEnv around DeviceGaitScheduleVecEnv: the rows are 10 clock columns wider than the env's "
                             "frames and the clock takes no sensor noise; put it inside, DeviceGaitScheduleVecEnv(DevicePerturbedVecEnv(env))")
        po = hasattr(venv, "obs_window")                    # the stacked frames; its finished rows hold the reset stack
        frame = venv.FRAME if po else venv.obs_dim
        window = venv.obs_window if po else 1
        step_seconds = float(venv.model.opt.timestep) * venv.frame_skip
        lo, hi = (int(round(float(s) / step_seconds)) for s in action_latency)
        if not 0 <= lo <= hi <= _abi.PERTURB_MAX_DELAY:
            raise ValueError(f"action_latency {tuple(action_latency)} s is {(lo, hi)} env-steps of {step_seconds} s: 0 <= lo <= hi <= "
                             f"{_abi.PERTURB_MAX_DELAY}")
        sim = venv._sim
        base = sim.env_index_base if env_index_base is None else env_index_base
        self.perturbation = Perturbation(venv.num_envs, frame, window, obs_noise, obs_bias, action_noise, (lo, hi),
                                         reset_action=list(sim.task.default_ctrl), done_row="reset" if po else "terminal", seed=seed,
                                         env_index_base=base, device=venv.device if device is None else device)
        super().__init__(venv, self.perturbation)
        self._delayed = torch.empty((venv.num_envs, _abi.NU), dtype=torch.float32, device=self.perturbation._torch_device())

    # -- device path ------------------------------------------------------------------------
    def step_tensor(self, actions, *args, **kwargs):
        """The wrapped env's ``step_tensor`` with its signature; the observations it fills come back perturbed in place."""
        stream = kwargs.get("stream")
        self.perturbation.perturb_actions(actions, out=self._delayed, stream=stream)
        if self._packed:
            packed = self.venv.step_tensor(self._delayed, *args, **kwargs)
            return self.perturbation.observe_packed(packed, stream=stream)
        bound = self._step_buffers(args, kwargs)
        self.venv.step_tensor(self._delayed, *args, **kwargs)
        self.perturbation.observe(bound["obs"], bound["done"], terminal_obs=bound.get("terminal_obs"), stream=stream)
        return None

    # -- NumPy cold path --------------------------------------------------------------------
    def reset(self):
        rows = self._upload(self.venv.reset())
        self.perturbation.begin(rows=rows)
        return rows.cpu().numpy()

    def step_async(self, actions):
        self.perturbation.perturb_actions(self._upload(actions), out=self._delayed)
        self.venv.step_async(self._delayed.cpu().numpy())

    def step_wait(self):
        """The host envs return a finished env's reset observation in ``obs`` and its last one in ``infos``; the device rows hold one
        of them (``done_row``).  The other travels beside it: the terminal stack as ``terminal_obs`` where the row is the reset stack;
        where the row is the terminal observation it goes through ``observe`` in the row's place and the reset observation (zeros)
        comes back as the env returned it."""
        obs, rew, done, infos = self.venv.step_wait()
        obs = np.array(obs, dtype=np.float32)
        finished = [i for i, _ in self._finished_with_terminal(done, infos)]
        reset_rows = self.perturbation.done_row == "reset"
        term = np.zeros_like(obs)
        for i in finished:
            term[i] = infos[i]["terminal_observation"]
        rows = obs.copy()
        if not reset_rows:
            rows[finished] = term[finished]
        t_rows = self._upload(rows)
        t_term = self._upload(term) if reset_rows and finished else None
        self.perturbation.observe(t_rows, self._upload(done, np.uint8), terminal_obs=t_term)
        rows = t_rows.cpu().numpy()
        term = t_term.cpu().numpy() if t_term is not None else rows
        for i in finished:
            info = dict(infos[i])
            info["terminal_observation"] = term[i].copy()
            infos[i] = info
        if not reset_rows:
            rows[finished] = obs[finished]
        return rows, rew, done, infos

    # -- checkpoint / resume ----------------------------------------------------------------
    def _layer_state(self):
        return self.perturbation.state()

    def _load_layer_state(self, state):
        self.perturbation.load_state(state)
