"""``GaitReward`` and ``DeviceGaitRewardVecEnv`` -- gait-shaped reward terms from the foot-contact sensor on rows that stay on the GPU
(``qg_gait_*`` of ``include/quadgym.h``, ``csrc/qg_gait.hip``): ``feet_air_time``, ``feet_slip``, ``feet_clearance``,
``touchdown_speed``, ``feet_contact_force``, ``body_contact`` and ``flight``, weighted, added to the env's reward and written as
component columns behind the env's own.

One launch of hand-written gfx950 code behind the env-step: it IS the sensor's advancing read of that env-step (forces, foot rows and
timers exactly as ``ContactSensor.read``) with the per-env reduction and the reward write in the same kernel -- do not also call
``sensor.read(advance=True)`` in that env-step.  PyTorch is plumbing only; there is no CPU path.  The handle has no per-env state of
its own: the gait timers are the sensor's and travel in the env's snapshot.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import GAIT_MAX_BASE_TERMS, GAIT_TERMS, QgGaitDesc, check          # (QgGaitDesc: re-exported)
from ._handle import Handle
from .envs.device_wrapper import STEP_BUFFERS, DeviceVecEnvWrapper, stack_layers

NTERMS = len(GAIT_TERMS)
THRESHOLDS = ("air_time_target", "clearance_target", "max_contact_force", "min_command_speed")


def term_weights(weights) -> list:
    """``[7]`` floats in the order of ``GAIT_TERMS`` from ``{name: w}`` (missing names weigh 0) or None (all 0).  An unknown name or a
    non-finite weight raises ``ValueError``."""
    weights = dict(weights or {})
    unknown = sorted(set(weights) - set(GAIT_TERMS))
    if unknown:
        raise ValueError(f"weights: unknown reward terms {unknown}: one of {', '.join(GAIT_TERMS)}")
    out = [float(weights.get(name, 0.0)) for name in GAIT_TERMS]
    for name, w in zip(GAIT_TERMS, out):
        if not np.isfinite(w):
            raise ValueError(f"weights[{name!r}] must be finite, got {w}")
    return out


class GaitReward(Handle):
    """Bound to ``sensor`` (a ``ContactSensor``; this is its ``Handle`` child, so it is destroyed before it).  The terms, the gate and
    the treatment of finished envs are defined in ``include/quadgym.h``."""

    _destroy = "qg_gait_destroy"
    TERMS = GAIT_TERMS

    def __init__(self, sensor, weights=None, air_time_target: float = 0.25, clearance_target: float = 0.05,
                 max_contact_force: float = 20.0, min_command_speed: float = 0.1):
        w = term_weights(weights)
        limits = dict(zip(THRESHOLDS, (air_time_target, clearance_target, max_contact_force, min_command_speed)))
        for name, value in limits.items():
            limits[name] = float(value)
            if not np.isfinite(limits[name]) or limits[name] < 0.0:
                raise ValueError(f"{name} must be finite and >= 0, got {value}")
        super().__init__(sensor.device, parent=sensor)
        self.sensor, self.num_envs = sensor, sensor.num_envs
        self.weights = dict(zip(GAIT_TERMS, w))
        for name, value in limits.items():
            setattr(self, name, value)
        self.desc = QgGaitDesc.make(w, **limits)
        self._create("qg_gait_create", sensor._h, C.byref(self.desc))

    def set_weights(self, weights):
        """New weights ``{name: w}`` for the launches that follow (missing names keep their weight); a captured graph keeps the
        weights it was captured with."""
        w = term_weights(dict(self.weights, **dict(weights)))
        check(self._lib.qg_gait_set_weights(self._h, (C.c_float * NTERMS)(*w)), "qg_gait_set_weights")
        self.weights = dict(zip(GAIT_TERMS, w))

    # -- device path ------------------------------------------------------------------------
    @staticmethod
    def _span(t, width, stride):
        lo = t.data_ptr()
        return lo, lo + 4 * ((t.shape[0] - 1) * stride + width)

    def step(self, done=None, reward=None, reward_out=None, components=None, base_components=None, command=None, advance: bool = True,
             body_force=None, feet=None, stream=None):
        """One launch on ``stream`` (torch's current stream by default), behind the env-step whose state it is to see.  Returns
        ``(components, reward_out)``, allocated unless passed.

        ``done``: uint8 / bool / float32 ``[N]`` at any positive stride or None; the envs it names get seven zeros and their reward
        unchanged.  ``reward`` (optional), ``reward_out`` (may be ``reward``): float32 ``[N]`` at any positive stride.
        ``base_components``: float32 ``[N, C0]``, ``C0 <= 25``, rows at a stride -- copied in front of the seven columns, so that
        ``components`` is ``[N, C0 + 7]`` (rows at a stride >= that).  The two may not overlap, unless ``base_components`` is
        ``components[:, :C0]`` itself.  ``command``: float32 ``[N, 2]``, rows at a stride, gates ``feet_air_time``.  ``advance``,
        ``body_force`` ``[N, 13, 3]`` and ``feet`` ``[N, 4, 12]`` (optional outputs) are ``ContactSensor.read``'s.  A bad argument
        raises ``ValueError`` before any launch."""
        import torch
        n, dev = self.num_envs, self._torch_device()
        # the caller's tensors first, every one of them; what is missing is allocated behind the checks
        d_ptr, kind, d_stride = self._done_arg(done)
        r_ptr, r_stride = None, 1
        if reward is not None:
            r_stride, r_ptr = self._check_vec(reward, (torch.float32,), "reward"), reward.data_ptr()
        o_stride = 1 if reward_out is None else self._check_vec(reward_out, (torch.float32,), "reward_out")
        b_ptr, b_stride, c0 = None, 0, 0
        if base_components is not None:
            if base_components.dim() != 2 or not 0 <= base_components.shape[1] <= GAIT_MAX_BASE_TERMS:
                raise ValueError(f"base_components: expected [N, C0] with C0 <= {GAIT_MAX_BASE_TERMS}, got {tuple(base_components.shape)}")
            c0 = int(base_components.shape[1])
            b_stride, b_ptr = self._check_rows(base_components, c0, "base_components"), base_components.data_ptr()
        c_stride = c0 + NTERMS
        if components is not None:
            c_stride = self._check_rows(components, c0 + NTERMS, "components")
            if c0 and not (b_ptr == components.data_ptr() and b_stride == c_stride):
                (a0, a1), (b0, b1) = self._span(base_components, c0, b_stride), self._span(components, c0 + NTERMS, c_stride)
                if a0 < b1 and b0 < a1:
                    raise ValueError("base_components and components overlap: allowed only where base_components is components[:, :C0]")
        m_ptr, m_stride = None, 2
        if command is not None:
            m_stride, m_ptr = self._check_rows(command, 2, "command"), command.data_ptr()
        self.sensor._check_outputs(body_force, feet)
        if reward_out is None:
            reward_out = torch.empty(n, device=dev, dtype=torch.float32)
        if components is None:
            components = torch.empty((n, c0 + NTERMS), device=dev, dtype=torch.float32)
        check(self._lib.qg_gait_reward_device(self._h, d_ptr, kind, d_stride, 1 if advance else 0, r_ptr, r_stride, reward_out.data_ptr(), o_stride,
                                            components.data_ptr(), c_stride, b_ptr, b_stride, c0, m_ptr, m_stride,
                                            body_force.data_ptr() if body_force is not None else None,
                                            feet.data_ptr() if feet is not None else None, self._stream_ptr(stream)), "qg_gait_reward_device")
        return components, reward_out


class DeviceGaitRewardVecEnv(DeviceVecEnvWrapper):
    """The gait terms around ``QuadrupedVecEnv``, ``WalkingQuadrupedVecEnv`` or ``POWalkingQuadrupedVecEnv`` (or a device-side wrapper
    around one): ``step_tensor`` runs the env's launch, then the gait launch on the same stream, and ``reward`` comes back shaped.
    The sensor is the env's (``venv.contact_sensor(force_threshold)``): the env's ``reset`` restarts its timers and the env's snapshot
    carries them, so this layer's own state is empty.  ``components``, if passed, is ``[N, len(venv.reward_keys) + 7]``: the env's
    columns, then the seven -- ``reward_keys`` lists them, so ``RewardMonitor.for_env(wrapper)`` works as it is.
    ``gate_on_command=True`` (the partially observable env only) gates ``feet_air_time`` on the newest frame's command columns, in
    m/s: around a ``DeviceVecNormalize`` with ``norm_obs=True`` it is refused at construction, before any handle exists (the order
    that works is ``DeviceVecNormalize(DeviceGaitRewardVecEnv(env, gate_on_command=True))``).  The
    NumPy ``step()`` is a cold path built for correctness: it returns shaped rewards and leaves ``last_gait_components [N, 7]``;
    ``infos`` stay the env's.  Every other attribute passes through to the wrapped env."""

    _snapshot_key = "gait_reward"
    PO_COMMAND = 23                        # the command's vx, vy in a partially observable frame (po_walking_quad.py:48-56)

    def __init__(self, venv, weights=None, force_threshold: float = 1.0, gate_on_command: bool = False, **options):
        if gate_on_command and not hasattr(venv, "obs_window"):
            raise ValueError("gate_on_command: only the partially observable env's observation holds the command")
        if gate_on_command and any(layer._snapshot_key == "normalizer" and layer.normalizer.norm_obs for layer in stack_layers(venv)):
            raise ValueError("gate_on_command around a DeviceVecNormalize that normalises observations: the gate would compare normalised "
                             "command columns with min_command_speed in m/s; put the gait terms inside, "
                             "DeviceVecNormalize(DeviceGaitRewardVecEnv(env, gate_on_command=True))")
        self.gait = GaitReward(venv.contact_sensor(force_threshold), weights, **options)
        super().__init__(venv, self.gait)
        self.gate_on_command = bool(gate_on_command)
        self.last_gait_components = None
        self._base = None                   # the env's own component columns of a step_tensor call, [N, len(venv.reward_keys)]

    @property
    def reward_keys(self):
        return list(self.venv.reward_keys) + list(GAIT_TERMS)

    def _command(self, obs):
        """The newest frame's (vx, vy) of the stacked observation, as a strided view."""
        if not self.gate_on_command:
            return None
        lo = (self.venv.obs_window - 1) * self.venv.FRAME + self.PO_COMMAND
        return obs[:, lo:lo + 2]

    # -- device path ------------------------------------------------------------------------
    def step_tensor(self, actions, *args, **kwargs):
        """The wrapped env's ``step_tensor`` with its signature; ``reward`` comes back shaped in place and ``components``, if passed,
        is ``[N, len(reward_keys)]``."""
        import torch
        stream = kwargs.get("stream")
        if self._packed:                                    # (obs, reward, done) rows; the plain env's step has no component buffer
            packed = self.venv.step_tensor(actions, *args, **kwargs)
            D = packed.shape[1] - 2
            self.gait.step(packed[:, D + 1], packed[:, D], packed[:, D], stream=stream)
            return packed
        bound = self._step_buffers(args, kwargs)
        wide = bound.get("components")
        if wide is None:
            self.venv.step_tensor(actions, *args, **kwargs)
            self.gait.step(bound["done"], bound["reward"], bound["reward"], command=self._command(bound["obs"]), stream=stream)
            return None
        c0 = len(self.venv.reward_keys)
        self.gait._check_rows(wide, c0 + NTERMS, "components")             # before the env's launch
        if self._base is None:
            self._base = torch.empty((self.num_envs, c0), device=self.gait._torch_device(), dtype=torch.float32)
        inner = dict(zip(STEP_BUFFERS, args), **kwargs)           # the positional buffers by name
        inner["components"] = self._base                    # the env writes contiguous rows; the gait launch copies them in front
        self.venv.step_tensor(actions, **inner)
        self.gait.step(bound["done"], bound["reward"], bound["reward"], wide, self._base, self._command(bound["obs"]), stream=stream)
        return None

    # -- NumPy cold path --------------------------------------------------------------------
    def reset(self):
        self.last_gait_components = None
        return self.venv.reset()

    def step_async(self, actions):
        self.venv.step_async(actions)

    def step_wait(self):
        obs, rew, done, infos = self.venv.step_wait()
        command = None
        if self.gate_on_command:
            command = self._command(self._upload(obs))
        comps, shaped = self.gait.step(self._upload(done, np.uint8), self._upload(rew), command=command)
        self.last_gait_components = comps.cpu().numpy()
        return obs, shaped.cpu().numpy(), done, infos

    # -- checkpoint / resume: nothing of its own ----------------------------------------------
    def _layer_state(self):
        return {}

    def _load_layer_state(self, state):
        pass

