"""``FusedMlpPolicy`` -- a tanh MLP policy (actor, optional critic, diagonal-Gaussian log-probability) evaluated in ONE launch of
hand-written gfx950 code (``qg_policy_*`` of ``include/quadgym.h``, ``csrc/qg_policy.hip``).

It reads the rows a step left on the device in place (a row stride is allowed) and writes what a PPO rollout collects: action,
log-probability, value.  A closed-loop step is then two launches: the policy and the env step.  PyTorch is plumbing
only: it owns the tensors and the stream.  There is no CPU path.
"""
from __future__ import annotations

import collections
import ctypes as C
import math

import numpy as np

from ._abi import DISTILL_LOSSES, QgAdamParams, QgDistillBatch, QgDistillParams, QgPolicyDesc, QgPpoBatch, QgPpoParams, check
from ._handle import Handle


def _np32(a):
    """A torch tensor or array-like as a float32 NumPy array (host copy)."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float32)


def flatten_layers(actor, log_std, critic=None):
    """The canonical flat parameter vector of ``include/quadgym.h``: the actor's layers in order, each ``W[out][in]`` row-major then
    ``b[out]``; ``log_std``; then the critic's layers in the same way."""
    parts = []
    for W, b in actor:
        parts += [_np32(W).ravel(), _np32(b).ravel()]
    parts.append(_np32(log_std).ravel())
    for W, b in (critic or []):
        parts += [_np32(W).ravel(), _np32(b).ravel()]
    return np.concatenate(parts).astype(np.float32)


def _sequential_layers(seq):
    """``[(W, b), ...]`` of a ``torch.nn.Sequential`` of ``Linear`` / ``Tanh``; the second value says whether it ends in ``Tanh``."""
    import torch
    layers, mods = [], list(seq)
    for i, m in enumerate(mods):
        if isinstance(m, torch.nn.Linear):
            if m.bias is None:
                raise ValueError("Linear layers need a bias")
            if i + 1 < len(mods) and not isinstance(mods[i + 1], torch.nn.Tanh):
                raise ValueError("every Linear but the last must be followed by Tanh (the only activation)")
            layers.append((m.weight, m.bias))
        elif not isinstance(m, torch.nn.Tanh):
            raise ValueError(f"unsupported module {type(m).__name__}: Linear and Tanh only")
        elif i == 0 or not isinstance(mods[i - 1], torch.nn.Linear):
            raise ValueError("Tanh must follow a Linear")
    return layers, bool(mods) and isinstance(mods[-1], torch.nn.Tanh)


class FusedMlpPolicy(Handle):
    """``obs_dim -> hidden[0] -> .. -> act_dim`` with tanh after every hidden layer; ``out_tanh`` puts a tanh on the action mean too
    (``False``: SB3's linear ``action_net``); ``value=True`` adds a critic tower with the same hidden sizes and one output.
    ``critic_obs=(offset, dim)`` makes the pair asymmetric: the actor reads columns ``[0, obs_dim)`` of a row, the critic columns
    ``[offset, offset + dim)`` of the same row (``privileged.py`` writes such rows), and its first layer is ``dim`` wide.

    Hidden widths are multiples of 16 up to 256, at most three of them; ``obs_dim <= 512``, ``act_dim <= 16``.  A new policy holds
    zeros; load parameters with ``load_layers`` / ``load_module`` / ``load_sb3_state_dict`` (host) or ``update_from`` (device,
    stream-ordered).  Outputs for non-finite observations are unspecified."""

    _destroy = "qg_policy_destroy"
    # rows per partial-sum slot of ``ppo_grad`` (32 tiles of 16 rows): a workgroup of its weight-gradient launch sums that many
    # consecutive rows, the reduce launch adds the slots in ascending order (QGG_SLOT_TILES of csrc/qg_policy.h)
    GRAD_TILE_ROWS = 16
    GRAD_SLOT_ROWS = 512
    # canonical elements per slot of ``adam_step``'s gradient norm: a workgroup sums the squares of that many consecutive elements in
    # float64, every workgroup of the update launch adds the slots in ascending order (QGA_SLOT of csrc/qg_policy.h)
    ADAM_SLOT = 2048
    asymmetric = False          # the critic reads a window of its own (critic_obs=...)
    _critic_obs = None

    @property
    def critic_obs(self):
        """``(offset, dim)``: the columns of a row the critic reads; ``(0, obs_dim)`` unless the policy is asymmetric."""
        return self._critic_obs if self._critic_obs is not None else (0, self.obs_dim)

    def __init__(self, obs_dim: int, hidden, act_dim: int, out_tanh: bool = False, value: bool = True, device: int = 0, critic_obs=None):
        super().__init__(device)
        self.obs_dim, self.act_dim, self.hidden = int(obs_dim), int(act_dim), tuple(int(h) for h in hidden)
        self.out_tanh, self.has_value = bool(out_tanh), bool(value)
        if len(self.hidden) > 3:
            raise ValueError("at most three hidden layers")
        self.desc = QgPolicyDesc.make(self.obs_dim, self.hidden, self.act_dim, self.out_tanh, self.has_value)
        if critic_obs is not None:
            if not self.has_value:
                raise ValueError("critic_obs: the policy was built with value=False")
            off, dim = (int(x) for x in critic_obs)
            self._create("qg_policy_create_asym", self.device, C.byref(self.desc), off, dim)
            self.n_params = int(self._lib.qg_policy_param_count_asym(C.byref(self.desc), dim))
        else:
            self._create("qg_policy_create", self.device, C.byref(self.desc))
            self.n_params = int(self._lib.qg_policy_param_count(C.byref(self.desc)))
        off, dim = C.c_int32(), C.c_int32()
        check(self._lib.qg_policy_critic_window(self._h, C.byref(off), C.byref(dim)), "qg_policy_critic_window")
        self._critic_obs = (off.value, dim.value)
        self.asymmetric = self._critic_obs != (0, self.obs_dim)     # the window (0, obs_dim) IS the symmetric policy, however it was asked for

    # -- parameters -------------------------------------------------------------------------
    def layer_shapes(self):
        """``(actor, critic)``: the ``(out, in)`` shapes of the weight matrices, in order."""
        def body(first):
            dims = (first,) + self.hidden
            return [(dims[i + 1], dims[i]) for i in range(len(self.hidden))]
        last = self.hidden[-1]
        return body(self.obs_dim) + [(self.act_dim, last)], (body(self.critic_obs[1]) + [(1, last)] if self.has_value else [])

    @staticmethod
    def param_layout(obs_dim, hidden, act_dim, value=True, critic_obs_dim=None):
        """``name -> (offset, shape)`` over the canonical flat vector of a policy of this description, in order: ``actor.0.weight``,
        ``actor.0.bias``, .., ``log_std``, ``critic.0.weight``, ..  (``k`` counts the Linear layers of a tower).  ``critic_obs_dim``:
        the input width of an asymmetric critic (None: the actor's).  Host arithmetic only."""
        hidden = tuple(int(h) for h in hidden)
        out, off = collections.OrderedDict(), 0
        for tower, last in (("actor", int(act_dim)), ("critic", 1))[:2 if value else 1]:
            dims = (int(obs_dim if tower == "actor" or critic_obs_dim is None else critic_obs_dim),) + hidden
            for k, (i, o) in enumerate(zip(dims, dims[1:] + (last,))):
                out[f"{tower}.{k}.weight"] = (off, (o, i))
                out[f"{tower}.{k}.bias"] = (off + o * i, (o,))
                off += o * i + o
            if tower == "actor":
                out["log_std"] = (off, (int(act_dim),))
                off += int(act_dim)
        return out

    def param_slices(self):
        """``param_layout`` of this policy: view ``params()``, a flat parameter tensor or the ``grad`` of ``ppo_grad`` per layer with
        ``flat[off:off + math.prod(shape)].view(shape)``."""
        return self.param_layout(self.obs_dim, self.hidden, self.act_dim, self.has_value, self.critic_obs[1])

    def set_params(self, flat):
        """The canonical flat vector from the host (synchronous)."""
        flat = np.ascontiguousarray(_np32(flat))
        if flat.shape != (self.n_params,):
            raise ValueError(f"expected {self.n_params} parameters, got shape {flat.shape}")
        check(self._lib.qg_policy_set_params(self._h, flat.ctypes.data), "qg_policy_set_params")

    def params(self):
        """The canonical flat vector as set (NumPy float32; waits for the device)."""
        out = np.empty(self.n_params, np.float32)
        check(self._lib.qg_policy_get_params(self._h, out.ctypes.data), "qg_policy_get_params")
        return out

    def load_layers(self, actor, log_std=None, critic=None):
        """``actor=[(W, b), ...]`` with ``W`` of shape ``(out, in)`` (torch's ``Linear.weight``), torch tensors or NumPy arrays;
        ``log_std`` defaults to zeros; ``critic`` likewise, required exactly when the policy has a value tower."""
        want_a, want_c = self.layer_shapes()
        critic = list(critic) if critic is not None else []
        if bool(critic) != self.has_value:
            raise ValueError("critic layers are required exactly when the policy was built with value=True")
        for name, layers, want in (("actor", list(actor), want_a), ("critic", critic, want_c)):
            if len(layers) != len(want):
                raise ValueError(f"{name}: expected {len(want)} layers, got {len(layers)}")
            for i, ((W, b), shape) in enumerate(zip(layers, want)):
                if tuple(_np32(W).shape) != shape or tuple(_np32(b).shape) != (shape[0],):
                    raise ValueError(f"{name} layer {i}: expected W {shape} and b ({shape[0]},), got {tuple(_np32(W).shape)}, {tuple(_np32(b).shape)}")
        if log_std is None:
            log_std = np.zeros(self.act_dim, np.float32)
        if _np32(log_std).shape != (self.act_dim,):
            raise ValueError(f"log_std must have shape ({self.act_dim},)")
        self.set_params(flatten_layers(actor, log_std, critic))

    def load_module(self, actor_seq, critic_seq=None, log_std=None):
        """From ``torch.nn.Sequential`` modules of ``Linear`` / ``Tanh``.  Whether the actor ends in ``Tanh`` must agree with
        ``out_tanh``; the critic ends in its ``Linear``."""
        actor, a_tanh = _sequential_layers(actor_seq)
        if a_tanh != self.out_tanh:
            raise ValueError(f"the actor module {'ends' if a_tanh else 'does not end'} in Tanh but out_tanh is {self.out_tanh}")
        critic = None
        if critic_seq is not None:
            critic, c_tanh = _sequential_layers(critic_seq)
            if c_tanh:
                raise ValueError("the critic's output layer is linear")
        self.load_layers(actor, log_std, critic)

    def load_sb3_state_dict(self, sd):
        """From a plain dict with the key names of Stable-Baselines3's ``ActorCriticPolicy.state_dict()`` as of its 2.x releases, for
        the default non-shared ``net_arch``: ``mlp_extractor.policy_net.{0,2,4}.{weight,bias}``, ``mlp_extractor.value_net.*``,
        ``action_net.{weight,bias}``, ``value_net.{weight,bias}``, ``log_std``.  The key names are taken from SB3's source; this
        has NOT been run against a real checkpoint (the package is not a dependency).  SB3's ``action_net`` is linear: ``out_tanh``
        must be False."""
        if self.out_tanh:
            raise ValueError("SB3's action_net is linear: build the policy with out_tanh=False")
        if self.asymmetric:
            raise ValueError("SB3's ActorCriticPolicy has no asymmetric critic: load an asymmetric policy with load_layers / load_module")

        def tower(prefix, head):
            return [(sd[f"{prefix}.{2 * i}.weight"], sd[f"{prefix}.{2 * i}.bias"]) for i in range(len(self.hidden))] + \
                [(sd[f"{head}.weight"], sd[f"{head}.bias"])]
        actor = tower("mlp_extractor.policy_net", "action_net")
        critic = tower("mlp_extractor.value_net", "value_net") if self.has_value else None
        self.load_layers(actor, sd["log_std"], critic)

    # -- device path ------------------------------------------------------------------------
    def _check_obs(self, t, n=None, what="obs", with_critic=False):
        """Rows of ``obs_dim`` columns at a row stride that reaches every column the launch reads: ``obs_dim`` where the critic is not
        launched, else the farther end of the two windows (the same number on a symmetric policy).  The tensor itself may be the
        actor's slice ``rows[:, :obs_dim]`` of wider rows, or the whole wide rows.  Returns ``(rows, row stride)``."""
        need = max(self.obs_dim, sum(self.critic_obs)) if (with_critic and self.has_value) else self.obs_dim
        shown = int(t.shape[1]) if t.dim() == 2 else 0      # the columns the caller's tensor itself vouches for
        if t.dim() == 2 and t.shape[1] > self.obs_dim and self.asymmetric:
            t = t[:, :self.obs_dim]                        # the wide rows: the same pointer and stride
        n, stride = super()._check_obs(t, n, what)
        if need > self.obs_dim:
            # the critic reads behind the actor's columns.  Several rows show it by their stride (and the memory under the LAST row must
            # be there too: a slice of wider rows shares their storage); a single row has no stride, so it must be the wide row itself
            window = f"the critic reads columns {self.critic_obs[0]} .. {sum(self.critic_obs)} of a row"
            if n == 1 and shown < need:
                raise ValueError(f"{what}: {window}; one row of {shown} columns does not hold them: pass the wide row")
            if n > 1 and stride < need:
                raise ValueError(f"{what}: {window}; the row stride {stride} is shorter")
            stride = max(stride, need)
            have = t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()
            if have < (n - 1) * stride + need:
                raise ValueError(f"{what}: {window}; the tensor's memory ends {(n - 1) * stride + need - have} floats before the last "
                                 f"row's: pass the wide rows, or their slice [:, :{self.obs_dim}]")
        return n, stride

    def update_from(self, params_tensor, stream=None):
        """The canonical flat vector from a device tensor, enqueued on ``stream`` (default: torch's current stream): forward passes
        enqueued later on that stream use it.  No host synchronisation."""
        import torch
        self._check_tensor(params_tensor, (self.n_params,), torch.float32)
        check(self._lib.qg_policy_set_params_device(self._h, params_tensor.data_ptr(), self._stream_ptr(stream)),
              "qg_policy_set_params_device")

    def launch_shape(self, n: int, value: bool = False):
        """``(waves per 16-env tile, output blocks per wave)`` of the kernel ``forward`` launches for ``n`` rows, with or without a
        value buffer.  Results do not depend on it; it tells a test or a timing which instantiation ran."""
        waves, blocks = C.c_int32(), C.c_int32()
        check(self._lib.qg_policy_launch_shape(self._h, int(n), int(bool(value)), C.byref(waves), C.byref(blocks)),
              "qg_policy_launch_shape")
        return waves.value, blocks.value

    def forward(self, obs, actions, eps=None, log_prob=None, value=None, stream=None):
        """One launch: ``actions[n, act_dim]`` (the mean, or ``mean + exp(log_std) * eps`` with standard-normal ``eps[n, act_dim]`` from
        the caller, not clipped), optionally ``log_prob[n]`` and ``value[n]``."""
        import torch
        n, stride = self._check_obs(obs, with_critic=value is not None)
        self._check_tensor(actions, (n, self.act_dim), torch.float32)
        if eps is not None:
            self._check_tensor(eps, (n, self.act_dim), torch.float32)
        if log_prob is not None:
            self._check_tensor(log_prob, (n,), torch.float32)
        if value is not None:
            if not self.has_value:
                raise ValueError("the policy was built with value=False")
            self._check_tensor(value, (n,), torch.float32)
        check(self._lib.qg_policy_forward_device(self._h, n, obs.data_ptr(), stride, eps.data_ptr() if eps is not None else None,
                                                 actions.data_ptr(), log_prob.data_ptr() if log_prob is not None else None,
                                                 value.data_ptr() if value is not None else None, self._stream_ptr(stream)),
              "qg_policy_forward_device")

    # -- the PPO update ---------------------------------------------------------------------
    def reserve_grad(self, max_batch: int):
        """Allocate what ``ppo_grad`` needs for minibatches of up to ``max_batch`` rows (waits for the device; not during a graph
        capture; call again to grow).  From here on every parameter update also repacks the transposed weights the pass reads."""
        check(self._lib.qg_policy_reserve_grad(self._h, int(max_batch)), "qg_policy_reserve_grad")

    def ppo_grad(self, batch, grad, stats=None, clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5, stream=None):
        """The PPO loss of one minibatch (SB3 2.x ``PPO.train``; ``include/quadgym.h`` states it) and its gradient, three launches on
        ``stream``: ``grad[n_params]`` in the canonical order, every element overwritten; ``stats[8]`` (optional) = loss, policy_loss,
        value_loss, entropy_loss, approx_kl, clip_fraction, 0, 0.  ``batch`` is a ``RolloutBufferSamples`` or anything with its six
        attributes (``old_values`` / ``returns`` may be None without a critic; ``old_values`` also without value clipping);
        ``observations`` may be row-strided.  Advantages are used as given."""
        import torch
        n, stride = self._check_obs(batch.observations, what="observations", with_critic=True)
        f32 = torch.float32
        self._check_tensor(batch.actions, (n, self.act_dim), f32, "actions")
        self._check_tensor(batch.old_log_prob, (n,), f32, "old_log_prob")
        self._check_tensor(batch.advantages, (n,), f32, "advantages")
        ptrs = dict(obs=batch.observations.data_ptr(), actions=batch.actions.data_ptr(), old_log_prob=batch.old_log_prob.data_ptr(),
                    advantages=batch.advantages.data_ptr())
        if self.has_value:
            if batch.returns is None or (batch.old_values is None and clip_range_vf is not None and clip_range_vf > 0):
                raise ValueError("a policy with a critic needs returns, and old_values when clip_range_vf is set")
            for name in ("old_values", "returns"):
                t = getattr(batch, name)
                if t is not None:
                    self._check_tensor(t, (n,), f32, name)
                    ptrs[name] = t.data_ptr()
        self._check_tensor(grad, (self.n_params,), f32, "grad")
        if stats is not None:
            self._check_tensor(stats, (8,), f32, "stats")
        params = QgPpoParams.make(clip_range, clip_range_vf, ent_coef, vf_coef)
        desc = QgPpoBatch.make(stride, **ptrs)
        check(self._lib.qg_policy_ppo_grad_device(self._h, C.byref(params), n, C.byref(desc), grad.data_ptr(),
                                                  stats.data_ptr() if stats is not None else None, self._stream_ptr(stream)),
              "qg_policy_ppo_grad_device")

    # -- teacher-student distillation -------------------------------------------------------
    DISTILL_STAT_NAMES = ("loss", "sq_err", "kl", "max_abs_err", "weight_sum")

    def distill_grad(self, obs, target_mean, grad, stats=None, *, loss="mse", coef=1.0, target_log_std=None, weights=None, stream=None):
        """The imitation loss of one minibatch (``include/quadgym.h`` states it) and its gradient, three launches on ``stream``, in the
        scratch of ``reserve_grad``: the action mean of this policy (the student) on ``obs`` against ``target_mean[n, act_dim]`` --
        what ``teacher.forward(rows, target_mean)`` wrote.  ``loss="mse"``: ``coef / n * sum_rows w * sum_a (mean - target)^2``;
        ``loss="kl"``: ``coef / n * sum_rows w * KL(N(target, exp(target_log_std)) || N(mean, exp(log_std)))`` with the teacher's
        ``target_log_std[act_dim]`` on the device.  ``weights[n]`` (optional) are the ``w``; the sum is divided by ``n``, not by their
        sum.  ``grad[n_params]`` in the canonical order, every element overwritten (the critic's entries, and ``log_std`` in MSE
        mode, with zeros); ``stats[8]`` (optional) = ``DISTILL_STAT_NAMES``, then zeros.  Only the actor's columns of a row are read:
        ``obs`` may be row-strided -- the slice ``rows[:, :obs_dim]`` of wider rows -- or the wide rows themselves."""
        import torch
        if loss not in DISTILL_LOSSES:
            raise ValueError(f"loss: expected one of {sorted(DISTILL_LOSSES)}, got {loss!r}")
        if not math.isfinite(coef):
            raise ValueError(f"coef must be finite, got {coef}")
        if obs.dim() == 2 and obs.shape[1] > self.obs_dim:
            obs = obs[:, :self.obs_dim]                    # the wide rows: the same pointer and stride
        n, stride = self._check_obs(obs)
        f32 = torch.float32
        self._check_tensor(target_mean, (n, self.act_dim), f32, "target_mean")
        ptrs = dict(obs=obs.data_ptr(), target_mean=target_mean.data_ptr())
        if loss == "kl":
            if target_log_std is None:
                raise ValueError('loss="kl" needs target_log_std, the teacher\'s log_std on the device')
            self._check_tensor(target_log_std, (self.act_dim,), f32, "target_log_std")
            ptrs["target_log_std"] = target_log_std.data_ptr()
        if weights is not None:
            self._check_tensor(weights, (n,), f32, "weights")
            ptrs["weights"] = weights.data_ptr()
        self._check_tensor(grad, (self.n_params,), f32, "grad")
        if stats is not None:
            self._check_tensor(stats, (8,), f32, "stats")
        params = QgDistillParams.make(loss, coef)
        desc = QgDistillBatch.make(stride, **ptrs)
        check(self._lib.qg_policy_distill_grad_device(self._h, C.byref(params), n, C.byref(desc), grad.data_ptr(),
                                                      stats.data_ptr() if stats is not None else None, self._stream_ptr(stream)),
              "qg_policy_distill_grad_device")

    # -- the optimiser ----------------------------------------------------------------------
    def reserve_adam(self):
        """Allocate the optimiser's state: both moments and the step count, zero, in device memory (waits for the device; not during
        a graph capture; a second call keeps the state).  ``reserve_grad`` is not needed for it."""
        check(self._lib.qg_policy_reserve_adam(self._h), "qg_policy_reserve_adam")

    def adam_step(self, grad, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.5, lr_tensor=None, params_out=None, stats=None,
                  stream=None):
        """``torch.nn.utils.clip_grad_norm_`` (``max_grad_norm=None`` or ``<= 0``: off) and one ``torch.optim.Adam`` step on the
        policy's own parameters, two launches on ``stream``; ``include/quadgym.h`` states the order of operations.  ``grad[n_params]``
        is read, not changed.  The operand images follow: the next ``forward`` / ``ppo_grad`` on the stream uses the new parameters,
        no ``update_from``.  ``lr_tensor`` (one float32 on the device) replaces ``lr`` and is read at every replay of a captured
        step; ``params_out[n_params]`` receives the new canonical vector; ``stats[4]`` = norm before clipping, clip coefficient, the
        step count after the step, the learning rate used."""
        import torch
        f32 = torch.float32
        self._check_tensor(grad, (self.n_params,), f32, "grad")
        if lr_tensor is not None:
            self._check_tensor(lr_tensor, (1,) if lr_tensor.dim() else (), f32, "lr_tensor")
        if params_out is not None:
            self._check_tensor(params_out, (self.n_params,), f32, "params_out")
            if params_out.data_ptr() == grad.data_ptr():
                raise ValueError("params_out must not be grad")
        if stats is not None:
            self._check_tensor(stats, (4,), f32, "stats")
        params = QgAdamParams.make(lr, betas, eps, max_grad_norm)
        check(self._lib.qg_policy_adam_update_device(self._h, C.byref(params), grad.data_ptr(),
                                                   lr_tensor.data_ptr() if lr_tensor is not None else None,
                                                   params_out.data_ptr() if params_out is not None else None,
                                                   stats.data_ptr() if stats is not None else None, self._stream_ptr(stream)),
              "qg_policy_adam_update_device")

    def adam_state(self):
        """``{"step": int, "exp_avg": float32[n_params], "exp_avg_sq": float32[n_params]}`` (NumPy; waits for the device): with
        ``params()`` what a checkpoint of the optimiser holds."""
        m, v, t = np.empty(self.n_params, np.float32), np.empty(self.n_params, np.float32), C.c_int64()
        check(self._lib.qg_policy_adam_get_state(self._h, m.ctypes.data, v.ctypes.data, C.byref(t)), "qg_policy_adam_get_state")
        return {"step": int(t.value), "exp_avg": m, "exp_avg_sq": v}

    def load_adam_state(self, state):
        """What ``adam_state`` returned, bit for bit (synchronous; after ``reserve_adam``)."""
        m, v = (np.ascontiguousarray(_np32(state[k])) for k in ("exp_avg", "exp_avg_sq"))
        if m.shape != (self.n_params,) or v.shape != (self.n_params,):
            raise ValueError(f"expected two moment vectors of {self.n_params} elements, got shapes {m.shape}, {v.shape}")
        check(self._lib.qg_policy_adam_set_state(self._h, m.ctypes.data, v.ctypes.data, int(state["step"])), "qg_policy_adam_set_state")

    def normalize_advantages(self, adv, out=None, stream=None):
        """SB3's ``normalize_advantage`` for one minibatch, one launch: ``(adv - adv.mean()) / (adv.std() + 1e-8)`` with both moments
        in float64 and one rounding.  ``out=None`` normalises ``adv`` in place; returns the tensor written."""
        import torch
        if adv.dim() != 1 or adv.shape[0] < 2:
            raise ValueError(f"adv: expected a vector of at least 2 rows, got shape {tuple(adv.shape)}")
        n = int(adv.shape[0])
        self._check_tensor(adv, (n,), torch.float32, "adv")
        if out is None:
            out = adv
        else:
            self._check_tensor(out, (n,), torch.float32, "out")
        check(self._lib.qg_policy_normalize_advantages_device(self._h, n, adv.data_ptr(), out.data_ptr(), self._stream_ptr(stream)),
              "qg_policy_normalize_advantages_device")
        return out
