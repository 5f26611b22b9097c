"""``RunningNormalizer`` and ``DeviceVecNormalize`` -- running observation and reward normalisation (SB3's ``VecNormalize``) on rows
that stay on the GPU (``qg_norm_*`` of ``include/quadgym.h``, ``csrc/qg_norm.hip``).

A training step is three small launches of hand-written gfx950 code on the caller's stream: f64 column moments of the batch, a
fixed-order combine with the running merge, and the normalise pass.  PyTorch is plumbing only: it owns the tensors and the stream.
There is no CPU path.  Outputs for non-finite inputs are unspecified (train the walking envs with ``nan_direction=False``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import QgNormDesc, check
from ._handle import Handle
from .envs.device_wrapper import DeviceVecEnvWrapper, base_env


class RunningNormalizer(Handle):
    """Per-column running mean / variance of the observations, rewards divided by the running standard deviation of the discounted
    return, both clipped: the semantics of Stable-Baselines3 2.x ``VecNormalize`` (restated in ``include/quadgym.h``), with the
    statistics in float64 on the device.  ``training = False`` freezes every word of the state.

    ``state_dict()`` uses the attribute names of SB3's ``VecNormalize`` (``obs_rms.mean`` ...); the names are taken from SB3's
    source and this has NOT been run against an SB3 pickle (the package is not a dependency)."""

    _destroy = "qg_norm_destroy"

    def __init__(self, num_envs: int, obs_dim: int, gamma: float = 0.99, epsilon: float = 1e-8, clip_obs: float = 10.0,
                 clip_reward: float = 10.0, norm_obs: bool = True, norm_reward: bool = True, device: int = 0):
        super().__init__(device)
        self.num_envs, self.obs_dim = int(num_envs), int(obs_dim)
        self.gamma, self.epsilon, self.clip_obs, self.clip_reward = float(gamma), float(epsilon), float(clip_obs), float(clip_reward)
        self.norm_obs, self.norm_reward = bool(norm_obs), bool(norm_reward)
        self.training = True
        self.desc = QgNormDesc.make(self.obs_dim, self.num_envs, gamma, epsilon, clip_obs, clip_reward, norm_obs, norm_reward)
        self._create("qg_norm_create", self.device, C.byref(self.desc))

    # -- device path ------------------------------------------------------------------------
    def step(self, obs, reward=None, done=None, obs_out=None, reward_out=None, stream=None):
        """One step over the ``num_envs`` rows: ``obs`` float32 ``[N, obs_dim]`` (strided rows allowed), ``reward`` float32 ``[N]``
        or None (an observation-only step), ``done`` uint8 / bool / float32 ``[N]`` or None.  ``obs_out`` / ``reward_out`` default to
        in place.  Returns ``(obs_out, reward_out)``."""
        import torch
        _, in_stride = self._check_obs(obs, self.num_envs)
        obs_out = obs if obs_out is None else obs_out
        _, out_stride = self._check_obs(obs_out, self.num_envs, "obs_out")
        r_ptr = ro_ptr = None
        r_stride = ro_stride = 1
        d_ptr, kind, d_stride = self._done_arg(None)
        if reward is not None:
            r_stride = self._check_vec(reward, (torch.float32,), "reward")
            reward_out = reward if reward_out is None else reward_out
            ro_stride = self._check_vec(reward_out, (torch.float32,), "reward_out")
            r_ptr, ro_ptr = reward.data_ptr(), reward_out.data_ptr()
            d_ptr, kind, d_stride = self._done_arg(done)
        elif done is not None or reward_out is not None:
            raise ValueError("done and reward_out need a reward")
        check(self._lib.qg_norm_step_device(self._h, self.num_envs, obs.data_ptr(), in_stride, obs_out.data_ptr(), out_stride, r_ptr,
                                            r_stride, ro_ptr, ro_stride, d_ptr, kind, d_stride, int(bool(self.training)),
                                            self._stream_ptr(stream)), "qg_norm_step_device")
        return obs_out, reward_out

    def step_packed(self, packed, out=None, stream=None):
        """The plain env's packed rows ``[N, obs_dim + 2]`` (obs, reward, done as float32) in one call, in place unless ``out`` is
        given (its done column is then copied over).  Returns the normalised packed tensor."""
        import torch
        D = self.obs_dim
        self._check_packed(packed, "packed")
        if out is not None:
            self._check_packed(out, "out")
        dst = packed if out is None else out
        self.step(packed[:, :D], packed[:, D], packed[:, D + 1], obs_out=dst[:, :D], reward_out=dst[:, D], stream=stream)
        if out is not None:
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
                out[:, D + 1].copy_(packed[:, D + 1])
        return dst

    def update_obs(self, obs, stream=None):
        """``obs_rms.update(obs)`` alone, for any number of rows (the observations of ``reset()``)."""
        n, stride = self._check_obs(obs)
        check(self._lib.qg_norm_update_obs_device(self._h, n, obs.data_ptr(), stride, self._stream_ptr(stream)), "qg_norm_update_obs_device")

    def normalize_obs(self, obs, out=None, stream=None):
        """Step 2 alone with the statistics as they stand, for any number of rows; in place unless ``out`` is given."""
        n, in_stride = self._check_obs(obs)
        out = obs if out is None else out
        _, out_stride = self._check_obs(out, n, "out")
        check(self._lib.qg_norm_apply_obs_device(self._h, n, obs.data_ptr(), in_stride, out.data_ptr(), out_stride, self._stream_ptr(stream)),
              "qg_norm_apply_obs_device")
        return out

    def reset_returns(self, stream=None):
        check(self._lib.qg_norm_reset_returns_device(self._h, self._stream_ptr(stream)), "qg_norm_reset_returns_device")

    # -- state ------------------------------------------------------------------------------
    def state_dict(self):
        """NumPy float64 (waits for the device): ``obs_rms.mean``, ``obs_rms.var``, ``obs_rms.count``, ``ret_rms.mean``,
        ``ret_rms.var``, ``ret_rms.count``, ``returns``."""
        mean, var = np.empty(self.obs_dim), np.empty(self.obs_dim)
        returns = np.empty(self.num_envs)
        s = [C.c_double() for _ in range(4)]
        check(self._lib.qg_norm_get_state(self._h, mean.ctypes.data, var.ctypes.data, *[C.addressof(x) for x in s], returns.ctypes.data),
              "qg_norm_get_state")
        return {"obs_rms.mean": mean, "obs_rms.var": var, "obs_rms.count": np.float64(s[0].value), "ret_rms.mean": np.float64(s[1].value),
                "ret_rms.var": np.float64(s[2].value), "ret_rms.count": np.float64(s[3].value), "returns": returns}

    def load_state_dict(self, sd):
        mean = np.ascontiguousarray(sd["obs_rms.mean"], dtype=np.float64)
        var = np.ascontiguousarray(sd["obs_rms.var"], dtype=np.float64)
        returns = np.ascontiguousarray(sd["returns"], dtype=np.float64)
        if mean.shape != (self.obs_dim,) or var.shape != (self.obs_dim,) or returns.shape != (self.num_envs,):
            raise ValueError(f"the state was taken from a normaliser of another shape: mean {mean.shape}, var {var.shape}, returns {returns.shape}")
        check(self._lib.qg_norm_set_state(self._h, mean.ctypes.data, var.ctypes.data, float(sd["obs_rms.count"]), float(sd["ret_rms.mean"]),
                                          float(sd["ret_rms.var"]), float(sd["ret_rms.count"]), returns.ctypes.data), "qg_norm_set_state")


class DeviceVecNormalize(DeviceVecEnvWrapper):
    """``VecNormalize`` around ``QuadrupedVecEnv``, ``WalkingQuadrupedVecEnv`` or ``POWalkingQuadrupedVecEnv`` whose ``step_tensor``
    stays on the device: the env's launch, then the normaliser's on the same stream.  Keyword options are ``RunningNormalizer``'s.
    The NumPy ``reset()`` / ``step()`` are a cold path built for correctness only (they upload the rows and run the same device
    calls).  Every other attribute passes through to the wrapped env.

    Terminal rows.  Where the wrapped stack reports an ``actor_obs_dim`` below its ``obs_dim`` (``DevicePrivilegedVecEnv`` inside:
    the statistics are over the wide row, ``terminal_obs`` and ``infos["terminal_observation"]`` stay at the actor's width), the
    terminal rows are normalised with the leading ``actor_obs_dim`` columns of the statistics: bit for bit what ``normalize_obs``
    gives on a wide row that holds them in front.  They go through a wide scratch allocated here, so a step allocates nothing.  A
    ``terminal_obs`` of any other width is refused before the env's launch.

    Refused at construction, before any handle exists: this wrapper around ``DevicePrivilegedVecEnv`` around the plain env (a packed
    step whose rows are not ``obs_dim`` wide: the wide rows travel beside the packed ones and would never be normalised).  There the
    normaliser goes INSIDE: ``DevicePrivilegedVecEnv(DeviceVecNormalize(env))`` -- actor columns normalised, privileged columns raw."""

    _snapshot_key = "normalizer"

    def __init__(self, venv, **options):
        if venv.packed_step and int(venv.obs_dim) != int(base_env(venv).obs_dim):
            raise ValueError(f"DeviceVecNormalize around a packed step whose rows are {int(base_env(venv).obs_dim)} + 2 wide while the stack's "
                             f"obs_dim is {int(venv.obs_dim)} (DevicePrivilegedVecEnv around the plain env): put the normaliser inside, "
                             "DevicePrivilegedVecEnv(DeviceVecNormalize(env)) -- actor columns normalised, privileged columns raw")
        device = options.pop("device", venv.device)
        self.normalizer = RunningNormalizer(venv.num_envs, venv.obs_dim, device=device, **options)
        super().__init__(venv, self.normalizer)
        self.old_obs = self.old_reward = None
        actor = getattr(venv, "actor_obs_dim", None)
        self.terminal_dim = int(venv.obs_dim) if actor is None else int(actor)      # the width of the stack's terminal rows
        self._term_wide = None
        if self.terminal_dim < self.normalizer.obs_dim:
            import torch
            self._term_wide = torch.zeros((self.num_envs, self.normalizer.obs_dim), device=self.normalizer._torch_device(), dtype=torch.float32)

    @property
    def training(self):
        return self.normalizer.training

    @training.setter
    def training(self, on):
        self.normalizer.training = bool(on)

    # -- device path ------------------------------------------------------------------------
    def step_tensor(self, actions, *args, **kwargs):
        """The wrapped env's ``step_tensor`` with its signature; the buffers it fills come back normalised in place."""
        stream = kwargs.get("stream")
        if self._packed:
            packed = self.venv.step_tensor(actions, *args, **kwargs)
            return self.normalizer.step_packed(packed, stream=stream)
        bound = self._step_buffers(args, kwargs)
        term = bound.get("terminal_obs")
        narrow = term is not None and self._check_terminal(term)                # before the env's launch
        if bound.get("obs") is not None:
            self.normalizer._check_obs(bound["obs"], self.normalizer.num_envs)
        self.venv.step_tensor(actions, *args, **kwargs)
        self.normalizer.step(bound["obs"], bound["reward"], bound["done"], stream=stream)
        if narrow:
            self._normalize_narrow(term, stream)
        elif term is not None:
            self.normalizer.normalize_obs(term, stream=stream)
        return None

    def _check_terminal(self, term):
        """True where ``term`` holds the stack's narrow terminal rows ``[N, terminal_dim]``, False where it is ``obs_dim`` wide (any
        number of rows, as ``normalize_obs`` takes them); any other tensor raises ``ValueError``."""
        nz = self.normalizer
        if self._term_wide is None or (term.dim() == 2 and term.shape[1] == nz.obs_dim):
            nz._check_obs(term, None, "terminal_obs")
            return False
        if term.dim() != 2 or term.shape[1] != self.terminal_dim or term.shape[0] > nz.num_envs:
            raise ValueError(f"terminal_obs: expected a float32 tensor of shape ({nz.num_envs}, {self.terminal_dim}) -- the stack's "
                             f"terminal rows stay at the actor's width -- or ({nz.num_envs}, {nz.obs_dim}), got {tuple(term.shape)}")
        nz._check_rows(term, self.terminal_dim, "terminal_obs", nz.ANY_ROWS)
        return True

    def _normalize_narrow(self, term, stream=None):
        """``term [n <= N, terminal_dim]`` in place with the leading columns of the statistics, through the wide scratch."""
        import torch
        n, O = term.shape[0], self.terminal_dim
        wide = self._term_wide[:n]
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.normalizer.device)):
            wide[:, :O].copy_(term)
            self.normalizer.normalize_obs(wide, stream=stream)
            term.copy_(wide[:, :O])
        return term

    # -- NumPy cold path --------------------------------------------------------------------
    def reset(self):
        obs = np.ascontiguousarray(self.venv.reset(), dtype=np.float32)
        self.old_obs = obs.copy()
        t = self._upload(obs)
        self.normalizer.reset_returns()
        if self.normalizer.training and self.normalizer.norm_obs:
            self.normalizer.update_obs(t)
        return self.normalizer.normalize_obs(t).cpu().numpy()

    def step_async(self, actions):
        self.venv.step_async(actions)

    def step_wait(self):
        obs, rew, done, infos = self.venv.step_wait()
        obs, rew = np.ascontiguousarray(obs, dtype=np.float32), np.ascontiguousarray(rew, dtype=np.float32)
        self.old_obs, self.old_reward = obs.copy(), rew.copy()
        t_obs, t_rew = self._upload(obs), self._upload(rew)
        self.normalizer.step(t_obs, t_rew, self._upload(done, np.uint8))
        rows = self._finished_with_terminal(done, infos)
        if rows:
            term = self._upload(np.stack([info["terminal_observation"] for _, info in rows]))
            if self._term_wide is not None and self._check_terminal(term):
                term = self._normalize_narrow(term).cpu().numpy()
            else:
                term = self.normalizer.normalize_obs(term).cpu().numpy()
            for k, (i, info) in enumerate(rows):
                info = dict(info)
                info["terminal_observation"] = term[k]
                infos[i] = info
        return t_obs.cpu().numpy(), t_rew.cpu().numpy(), done, infos

    def get_original_obs(self):
        return None if self.old_obs is None else self.old_obs.copy()

    def get_original_reward(self):
        return None if self.old_reward is None else self.old_reward.copy()

    # -- checkpoint / resume ----------------------------------------------------------------
    def _layer_state(self):
        return self.normalizer.state_dict()

    def _load_layer_state(self, state):
        self.normalizer.load_state_dict(state)

    def snapshot(self):
        return dict(super().snapshot(), training=self.normalizer.training)

    def restore(self, snap):
        super().restore(snap)
        self.normalizer.training = bool(snap.get("training", True))
