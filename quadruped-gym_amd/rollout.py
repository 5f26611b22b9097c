"""``DeviceRolloutBuffer`` -- SB3's ``RolloutBuffer`` for a collection loop that never leaves the GPU (``qg_rollout_*`` of
``include/quadgym.h``, ``csrc/qg_rollout.hip``): the record of a step, GAE over the filled slots and the gather of a minibatch are one
launch of hand-written gfx950 code each, on the caller's stream.  The cursor lives in device memory, so a hipGraph of ONE closed-loop
step fills the K slots when it is replayed K times.  PyTorch is plumbing only: it owns the storage tensors and the stream.  There is
no CPU path.
"""
from __future__ import annotations

import collections
import ctypes as C

from ._abi import QgRolloutBatch, QgRolloutDesc, QgRolloutInfo, QgRolloutStep, QgRolloutStorage, check
from ._handle import Handle

# SB3's RolloutBufferSamples
RolloutBufferSamples = collections.namedtuple("RolloutBufferSamples",
                                              ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns"])


class DeviceRolloutBuffer(Handle):
    """Storage under SB3's names -- ``observations [K + 1, N, obs_dim]`` (slot ``t`` is what the policy saw at step ``t``, slot ``pos``
    the observation after the last recorded step), ``actions [K, N, act_dim]``, ``log_probs``, ``values``, ``rewards``, ``advantages``,
    ``returns [K, N]`` float32 and ``dones [K, N]`` uint8 -- as torch tensors this object owns, written only by the library's launches.
    The semantics of every call are stated in ``include/quadgym.h``."""

    _destroy = "qg_rollout_destroy"

    def __init__(self, num_envs: int, n_steps: int, obs_dim: int, act_dim: int, gamma: float = 0.99, gae_lambda: float = 0.95,
                 device: int = 0):
        super().__init__(device)
        import torch
        self.num_envs, self.n_steps, self.obs_dim, self.act_dim = int(num_envs), int(n_steps), int(obs_dim), int(act_dim)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.desc = QgRolloutDesc.make(self.num_envs, self.n_steps, self.obs_dim, self.act_dim, gamma, gae_lambda)
        if min(self.num_envs, self.n_steps, self.obs_dim, self.act_dim) < 1:
            raise ValueError("num_envs, n_steps, obs_dim and act_dim must be >= 1")
        K, n = self.n_steps, self.num_envs
        dev = self._torch_device()
        f32 = dict(device=dev, dtype=torch.float32)
        self.observations = torch.zeros((K + 1, n, self.obs_dim), **f32)
        self.actions = torch.zeros((K, n, self.act_dim), **f32)
        self.log_probs, self.values, self.rewards = torch.zeros((K, n), **f32), torch.zeros((K, n), **f32), torch.zeros((K, n), **f32)
        self.advantages, self.returns = torch.zeros((K, n), **f32), torch.zeros((K, n), **f32)
        self.dones = torch.zeros((K, n), device=dev, dtype=torch.uint8)
        self.storage = QgRolloutStorage.make(obs=self.observations.data_ptr(), actions=self.actions.data_ptr(),
                                             log_prob=self.log_probs.data_ptr(), values=self.values.data_ptr(),
                                             rewards=self.rewards.data_ptr(), advantages=self.advantages.data_ptr(),
                                             returns=self.returns.data_ptr(), dones=self.dones.data_ptr())
        self._create("qg_rollout_create", self.device, C.byref(self.desc), C.byref(self.storage))
        self._count = 0                                     # calls of add() since begin(), capped at K: the CALLER's count
        self._batch = {}                                    # batch size -> reusable output tensors of get()

    # -- collection -------------------------------------------------------------------------
    def begin(self, obs=None, stream=None):
        """Start a rollout: the cursor goes to 0 and slot 0 takes ``obs`` (float32 ``[N, obs_dim]``, strided rows allowed).  Without
        ``obs`` the observation after the last recorded step is carried over: collection continues where it stopped."""
        ptr, stride = None, self.obs_dim
        if obs is not None:
            _, stride = self._check_obs(obs, self.num_envs)
            ptr = obs.data_ptr()
        check(self._lib.qg_rollout_begin_device(self._h, ptr, stride, self._stream_ptr(stream)), "qg_rollout_begin_device")
        self._count = 0

    def add(self, next_obs, actions, log_prob, value, reward, done, trunc_value=None, episode_reward=None, stream=None):
        """Record one env-step, after the env has stepped: ``actions [N, act_dim]``, ``log_prob`` and ``value [N]`` are what the policy
        returned for the observation in the current slot, ``reward [N]`` float32 and ``done [N]`` (uint8 / bool / float32) what the env
        returned, ``next_obs [N, obs_dim]`` the observation after the step.  ``trunc_value``: V(terminal observation) where the time
        limit truncated the episode, 0 elsewhere.  ``episode_reward``: what the episode statistics add up instead of ``reward``."""
        import torch
        f32 = (torch.float32,)
        _, o_stride = self._check_obs(next_obs, self.num_envs, "next_obs")
        self._check_tensor(actions, (self.num_envs, self.act_dim), torch.float32, "actions")
        self._check_tensor(log_prob, (self.num_envs,), torch.float32, "log_prob")
        self._check_tensor(value, (self.num_envs,), torch.float32, "value")
        r_stride = self._check_vec(reward, f32, "reward")
        d_ptr, d_kind, d_stride = self._done_arg(done)
        s = QgRolloutStep.make(next_obs=next_obs.data_ptr(), next_obs_stride=o_stride, actions=actions.data_ptr(),
                               log_prob=log_prob.data_ptr(), value=value.data_ptr(), reward=reward.data_ptr(), reward_stride=r_stride,
                               done=d_ptr, done_stride=d_stride, done_kind=d_kind)
        if trunc_value is not None:
            self._check_tensor(trunc_value, (self.num_envs,), torch.float32, "trunc_value")
            s.trunc_value = trunc_value.data_ptr()
        if episode_reward is not None:
            s.episode_reward_stride = self._check_vec(episode_reward, f32, "episode_reward")
            s.episode_reward = episode_reward.data_ptr()
        check(self._lib.qg_rollout_add_device(self._h, C.byref(s), self._stream_ptr(stream)), "qg_rollout_add_device")
        self._count = min(self._count + 1, self.n_steps)

    def add_packed(self, rows, actions, log_prob, value, trunc_value=None, episode_reward=None, stream=None):
        """``add`` for the plain env's packed rows ``[N, obs_dim + 2]`` (obs, reward, done as float32) where the step left them."""
        D = self.obs_dim
        self._check_packed(rows, "rows")
        self.add(rows[:, :D], actions, log_prob, value, rows[:, D], rows[:, D + 1], trunc_value=trunc_value,
                 episode_reward=episode_reward, stream=stream)

    @property
    def last_obs(self):
        """A view of slot ``pos`` of ``observations``: the observation after the last recorded step, which the critic turns into
        ``last_values``.  ``pos`` here is this object's count of ``add`` calls since ``begin`` (capped at ``n_steps``) -- the CALLER's
        count, not the device's: after replaying a captured ``add``, index ``observations`` by the number of replays instead."""
        return self.observations[self._count]

    def compute_returns_and_advantage(self, last_values, stream=None):
        """GAE over the filled slots into ``advantages`` and ``returns`` (one launch); ``last_values [N]`` float32."""
        import torch
        self._check_tensor(last_values, (self.num_envs,), torch.float32, "last_values")
        check(self._lib.qg_rollout_compute_device(self._h, last_values.data_ptr(), self._stream_ptr(stream)), "qg_rollout_compute_device")

    # -- minibatches ------------------------------------------------------------------------
    def _outputs(self, B):
        import torch
        if B not in self._batch:
            f32 = dict(device=self._torch_device(), dtype=torch.float32)
            self._batch[B] = RolloutBufferSamples(torch.empty((B, self.obs_dim), **f32), torch.empty((B, self.act_dim), **f32),
                                                  *[torch.empty(B, **f32) for _ in range(4)])
        return self._batch[B]

    def sample(self, idx, out=None, stream=None):
        """The samples ``idx`` (int64 ``[B]`` on the device; flat sample ``t * N + i``) in one launch.  ``out``: a
        ``RolloutBufferSamples`` of output tensors, a field None to skip it; default: reusable tensors of this object for that ``B``.
        An index outside the filled slots gives a row of zeros and counts in ``info()['bad_index']``."""
        import torch
        if not idx.is_cuda or idx.device.index != self.device:
            raise ValueError(f"idx must live on cuda:{self.device}")
        if idx.dim() != 1 or idx.shape[0] < 1 or idx.dtype != torch.int64 or not idx.is_contiguous():
            raise ValueError(f"idx: expected a contiguous int64 tensor of shape (B,), B >= 1, got {idx.dtype} {tuple(idx.shape)}")
        B = int(idx.shape[0])
        out = self._outputs(B) if out is None else RolloutBufferSamples(*out)
        b = QgRolloutBatch.make()
        for field, name, width in (("obs", "observations", self.obs_dim), ("actions", "actions", self.act_dim), ("old_values", "old_values", 0),
                                   ("old_log_prob", "old_log_prob", 0), ("advantages", "advantages", 0), ("returns", "returns", 0)):
            t = getattr(out, name)
            if t is None:
                continue
            self._check_tensor(t, (B, width) if width else (B,), torch.float32, f"out.{name}")
            setattr(b, field, t.data_ptr())
        check(self._lib.qg_rollout_gather_device(self._h, idx.data_ptr(), B, C.byref(b), self._stream_ptr(stream)), "qg_rollout_gather_device")
        return out

    def get(self, batch_size=None, generator=None):
        """One pass over the filled slots in minibatches of ``batch_size`` (the final short one included; None: one batch): one
        ``torch.randperm`` on the device per pass, one launch per minibatch.  The number of filled slots is the DEVICE's cursor
        (``info()``: waits for the device), so a buffer filled by graph replays is read in full.  The yielded tensors are reused by
        the next pass."""
        import torch
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        total = self.info()["pos"] * self.num_envs
        if total < 1:
            raise ValueError("the buffer is empty: nothing has been added since begin()")
        batch_size = total if batch_size is None else int(batch_size)
        perm = torch.randperm(total, device=self._torch_device(), generator=generator)
        for start in range(0, total, batch_size):
            yield self.sample(perm[start:start + batch_size])

    # -- bookkeeping ------------------------------------------------------------------------
    def info(self):
        """``{'pos', 'overflow', 'bad_index'}`` as the device has them (waits for the device; not during a capture)."""
        i = QgRolloutInfo()
        check(self._lib.qg_rollout_get_info(self._h, C.byref(i)), "qg_rollout_get_info")
        return {"pos": int(i.pos), "overflow": int(i.overflow), "bad_index": int(i.bad_index)}

    def episode_stats(self, clear=True):
        """SB3's ``ep_rew_mean`` and ``ep_len_mean`` over the episodes finished since the last clear, and their number ``episodes``
        (the means are NaN while no episode has finished).  Waits for the device.  ``clear`` keeps the running episodes."""
        rs, ls, cs = C.c_double(), C.c_int64(), C.c_int64()
        check(self._lib.qg_rollout_episode_stats(self._h, C.byref(rs), C.byref(ls), C.byref(cs), int(bool(clear))), "qg_rollout_episode_stats")
        n = int(cs.value)
        nan = float("nan")
        return {"ep_rew_mean": rs.value / n if n else nan, "ep_len_mean": ls.value / n if n else nan, "episodes": n,
                "return_sum": rs.value, "length_sum": int(ls.value)}
