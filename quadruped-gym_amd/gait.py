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
import functools

import numpy as np

from . import shaped
from ._abi import GAIT_MAX_BASE_TERMS, GAIT_TERMS, QgGaitDesc, check          # (GAIT_MAX_BASE_TERMS, QgGaitDesc: re-exported)
from ._handle import Handle
from .envs.device_wrapper import STEP_BUFFERS, DeviceVecEnvWrapper
from .envs.device_wrapper import stack_layers                                  # (re-exported)

NTERMS = len(GAIT_TERMS)
THRESHOLDS = ("air_time_target", "clearance_target", "max_contact_force", "min_command_speed")
term_weights = functools.partial(shaped.term_weights, terms=GAIT_TERMS)       # ``[7]`` floats in the order of ``GAIT_TERMS``


class GaitReward(shaped.ShapedReward, Handle):
    """Bound to ``sensor`` (a ``ContactSensor``; this is its ``Handle`` child, so it is destroyed before it).  The terms, the gate and
    the treatment of finished envs are defined in ``include/quadgym.h``."""

    _destroy = "qg_gait_destroy"
    _abi_prefix = "qg_gait"
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

    # -- device path ------------------------------------------------------------------------
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
        done3, rows11, components, reward_out = self._shaped_args(done, reward, reward_out, components, base_components, command,
                                                                  lambda: self.sensor._check_outputs(body_force, feet))
        check(self._lib.qg_gait_reward_device(self._h, *done3, 1 if advance else 0, *rows11, body_force.data_ptr() if body_force is not None else None,
                                            feet.data_ptr() if feet is not None else None, self._stream_ptr(stream)), "qg_gait_reward_device")
        return components, reward_out


class DeviceGaitRewardVecEnv(shaped.CommandGated, DeviceVecEnvWrapper):
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

    def __init__(self, venv, weights=None, force_threshold: float = 1.0, gate_on_command: bool = False, **options):
        self._check_gate(venv, gate_on_command,
                         "put the gait terms inside, DeviceVecNormalize(DeviceGaitRewardVecEnv(env, gate_on_command=True))")
        self.gait = GaitReward(venv.contact_sensor(force_threshold), weights, **options)
        super().__init__(venv, self.gait)
        self.gate_on_command = bool(gate_on_command)
        self.last_gait_components = None
        self._base = None                   # the env's own component columns of a step_tensor call, [N, len(venv.reward_keys)]

    @property
    def reward_keys(self):
        return list(self.venv.reward_keys) + list(GAIT_TERMS)

    # -- device path ------------------------------------------------------------------------
    def step_tensor(self, actions, *args, **kwargs):
        """The wrapped env's ``step_tensor`` with its signature; ``reward`` comes back shaped in place and ``components``, if passed,
        is ``[N, len(reward_keys)]``."""
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
        inner = dict(zip(STEP_BUFFERS, args), **kwargs)           # the positional buffers by name
        inner["components"] = self._rows("_base", c0)       # the env writes contiguous rows; the gait launch copies them in front
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

