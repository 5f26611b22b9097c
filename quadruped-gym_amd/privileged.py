"""``PrivilegedState`` and ``DevicePrivilegedVecEnv`` -- the simulator's truth as the input of an asymmetric critic, on rows that stay
on the GPU (``qg_priv_*`` of ``include/quadgym.h``, ``csrc/qg_priv.hip``): one launch writes, per env, the joint row
``[ actor observation (O) | privileged state (85) ]`` -- the observation copied bit for bit in front, and behind it the unlagged base
velocity, gravity direction, joint state, servo activations, foot contacts, forces and heights, the env's dynamics row, the wrench the
next env-step applies to the base (the scheduled push included) and the episode time.

One launch of hand-written gfx950 code behind the env-step; it only reads the simulator's state.  PyTorch is plumbing only; there is
no CPU path.  The layer has no per-env state: nothing to snapshot.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import PRIV_COLUMNS, PRIV_DIM, QgContactDesc, check
from .envs.device_wrapper import STEP_BUFFERS, DeviceVecEnvWrapper
from .envs.spaces import Box
from .task_layers import _TaskLayer


class PrivilegedState(_TaskLayer):
    """Bound to ``sim`` (its ``Handle`` child, so it is destroyed before it).  ``force_threshold`` (N) is the contact sensor's: a body
    touches where the vertical ground force on it exceeds it."""

    _destroy = "qg_priv_destroy"
    _abi_prefix = "qg_priv"
    DIM = PRIV_DIM
    COLUMNS = PRIV_COLUMNS

    def __init__(self, sim, force_threshold: float = 0.0):
        force_threshold = float(force_threshold)
        if not np.isfinite(force_threshold) or force_threshold < 0.0:
            raise ValueError(f"force_threshold must be finite and >= 0, got {force_threshold}")
        super().__init__(sim.device, parent=sim)
        self.num_envs = sim.n
        self.force_threshold = force_threshold
        self._create("qg_priv_create", sim._h, C.byref(QgContactDesc.make(force_threshold)))      # qg_priv_desc: the same fields

    @classmethod
    def column(cls, name) -> slice:
        """The columns of ``name`` (one of ``COLUMNS``) within the 85."""
        for key, first, width in cls.COLUMNS:
            if key == name:
                return slice(first, first + width)
        raise KeyError(name)

    def read(self, out, obs=None, stream=None):
        """One launch on ``stream`` (torch's current stream by default), behind the env-step whose state it is to see.  ``out``:
        float32 ``[N, O + 85]`` whose rows are contiguous, at any row stride (a column slice of a wider buffer; columns behind
        ``O + 85`` are not written); ``obs``: float32 ``[N, O]`` rows at a stride, copied to ``out[:, :O]``, or None (``O = 0``).  The
        two may not overlap.  A bad argument raises ``ValueError`` before any launch.  Returns ``out``."""
        o_ptr, o_stride, width = None, 0, 0
        if obs is not None:
            if obs.dim() != 2:
                raise ValueError(f"obs: expected a float32 tensor of shape ({self.num_envs}, O), got {tuple(obs.shape)}")
            width = int(obs.shape[1])
            o_stride, o_ptr = self._check_rows(obs, width, "obs"), obs.data_ptr()
        out_stride = self._check_rows(out, width + PRIV_DIM, "out")
        if obs is not None and width:
            a0, a1 = o_ptr, o_ptr + 4 * ((self.num_envs - 1) * o_stride + width)
            b0, b1 = out.data_ptr(), out.data_ptr() + 4 * ((self.num_envs - 1) * out_stride + width + PRIV_DIM)
            if a0 < b1 and b0 < a1:
                raise ValueError("obs and out overlap")
        check(self._lib.qg_priv_read_device(self._h, o_ptr, o_stride, width, out.data_ptr(), out_stride, self._stream_ptr(stream)),
              "qg_priv_read_device")
        return out

    def read_host(self):
        """``[N, 85]`` as a NumPy array: synchronous."""
        out = np.empty((self.num_envs, PRIV_DIM), np.float32)
        check(self._lib.qg_priv_read(self._h, out.ctypes.data), "qg_priv_read")
        return out


class DevicePrivilegedVecEnv(DeviceVecEnvWrapper):
    """The joint row around ``QuadrupedVecEnv``, ``WalkingQuadrupedVecEnv`` or ``POWalkingQuadrupedVecEnv`` (or a device-side wrapper
    around one): ``obs_dim`` / ``observation_space`` are ``actor_obs_dim + 85``; ``step_tensor`` runs the env's launch into the
    wrapper's own ``[N, O]`` buffer, then the one pack launch into the caller's ``[N, O + 85]`` rows, on the same stream.

    The privileged columns describe the state as it stands after the step: for a finished env that was auto-reset, the new episode's
    first state.  ``terminal_obs`` and ``infos["terminal_observation"]`` therefore stay at the actor's width ``O``: the terminal
    state's privileged columns no longer exist when the step returns.

    Stacking order: ``DevicePerturbedVecEnv`` goes INSIDE this wrapper (noise, bias and latency on the actor's columns only; the
    privileged columns stay clean; around this wrapper it is refused at construction), ``DeviceVecNormalize`` OUTSIDE around the
    walking envs (statistics over the wide row; it normalises the ``O``-wide terminal rows with the leading ``O`` columns of its
    statistics).  Around the plain env, whose packed step keeps the wide rows apart, the normaliser goes inside --
    ``DevicePrivilegedVecEnv(DeviceVecNormalize(env))``: actor columns normalised, privileged columns raw -- and is refused outside.
    The NumPy ``reset()`` / ``step()`` are a cold path built for correctness: they return wide rows.  Every other attribute passes
    through to the wrapped env."""

    _snapshot_key = "privileged"
    privileged_dim = PRIV_DIM

    def __init__(self, venv, force_threshold: float = 0.0):
        self.privileged = venv.privileged_state(force_threshold)
        super().__init__(venv, self.privileged)
        self.actor_obs_dim = int(venv.obs_dim)
        self.obs_dim = self.actor_obs_dim + PRIV_DIM
        self.observation_space = Box(low=-np.inf, high=np.inf, shape=(self.obs_dim,), dtype=np.float32)
        self._narrow = None                 # the env's own rows of a step_tensor call: [N, O], or packed [N, O + 2]
        self.wide_rows = None               # the packed step's wide rows where the caller passed none

    def _buffer(self, width):
        import torch
        if self._narrow is None or self._narrow.shape[1] != width:
            self._narrow = torch.empty((self.num_envs, width), device=self.privileged._torch_device(), dtype=torch.float32)
        return self._narrow

    # -- device path ------------------------------------------------------------------------
    def step_tensor(self, actions, *args, wide=None, **kwargs):
        """The wrapped env's ``step_tensor`` with its signature, ``obs`` being ``[N, O + 85]``.  Around the plain env (packed
        ``[N, O + 2]`` rows: obs, reward, done) the packed rows come back as they do from the env and the wide rows go to the extra
        keyword ``wide`` (``[N, O + 85]``; the wrapper's own ``wide_rows`` where None)."""
        import torch
        stream = kwargs.get("stream")
        O = self.actor_obs_dim
        if self._packed:
            if wide is None:
                if self.wide_rows is None:
                    self.wide_rows = torch.empty((self.num_envs, self.obs_dim), device=self.privileged._torch_device(), dtype=torch.float32)
                wide = self.wide_rows
            self.privileged._check_rows(wide, self.obs_dim, "wide")             # before the env's launch
            packed = self.venv.step_tensor(actions, *args, **kwargs)
            self.privileged.read(wide, packed[:, :O], stream=stream)
            return packed
        if wide is not None:
            raise ValueError("wide: only the packed step takes it; this env's step_tensor fills obs [N, O + 85]")
        bound = self._step_buffers(args, kwargs)
        if "obs" not in bound:
            raise ValueError("step_tensor: obs is required")
        self.privileged._check_rows(bound["obs"], self.obs_dim, "obs")         # before the env's launch
        inner = dict(zip(STEP_BUFFERS, args), **kwargs)           # the positional buffers by name
        inner["obs"] = self._buffer(O)                      # the env writes contiguous rows; the pack launch copies them in front
        self.venv.step_tensor(actions, **inner)
        self.privileged.read(bound["obs"], inner["obs"], stream=stream)
        return None

    # -- NumPy cold path --------------------------------------------------------------------
    def _widen(self, obs):
        import torch
        wide = torch.empty((self.num_envs, self.obs_dim), device=self.privileged._torch_device(), dtype=torch.float32)
        self.privileged.read(wide, self._upload(obs))
        return wide.cpu().numpy()

    def reset(self):
        return self._widen(self.venv.reset())

    def step_async(self, actions):
        self.venv.step_async(actions)

    def step_wait(self):
        obs, rew, done, infos = self.venv.step_wait()
        return self._widen(obs), rew, done, infos

    # -- checkpoint / resume: nothing of its own ----------------------------------------------
    def _layer_state(self):
        return {}

    def _load_layer_state(self, state):
        pass
