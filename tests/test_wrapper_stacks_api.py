"""The orders of the device-side wrappers without a GPU: an order that cannot work is refused at construction with a ValueError that
names the order that does, BEFORE any handle is created (the layer classes are replaced by recorders here: a refusal that comes after
one was asked for fails), the orders that work get as far as their handle, and a terminal_obs of a width the normaliser cannot take is
refused before the env's launch.  Stub envs hold what the wrappers read of an env before they reach the library."""
from types import SimpleNamespace

import pytest

from quadruped_gym_amd import gait, normalize, perturb
from quadruped_gym_amd.envs.device_wrapper import DeviceVecEnvWrapper
from quadruped_gym_amd.gait import DeviceGaitRewardVecEnv
from quadruped_gym_amd.normalize import DeviceVecNormalize, RunningNormalizer
from quadruped_gym_amd.perturb import DevicePerturbedVecEnv
from quadruped_gym_amd.privileged import DevicePrivilegedVecEnv

N = 8


class _Reached(Exception):
    """A wrapper's constructor got as far as creating its layer's handle."""


class _Env:
    """What the wrappers read of a batched env before they create a handle.  ``handles`` lists what was asked of it."""

    num_envs, device, frame_skip = N, 0, 4

    def __init__(self, obs_dim=33, packed_step=False, **extra):
        self.obs_dim, self.packed_step = obs_dim, packed_step
        self.model = SimpleNamespace(opt=SimpleNamespace(timestep=0.002))
        self._sim = SimpleNamespace(env_index_base=0, task=SimpleNamespace(default_ctrl=[0.0] * 12))
        self.reward_keys = ["alive_bonus"]
        self.handles = []
        self.launches = 0
        self.__dict__.update(extra)

    def contact_sensor(self, force_threshold=0.0):
        self.handles.append("contact")
        return SimpleNamespace(device=0, num_envs=N, _h=None)

    def privileged_state(self, force_threshold=0.0):
        self.handles.append("privileged")
        return SimpleNamespace(device=0, num_envs=N, _h=None)

    def step_tensor(self, *args, **kwargs):
        self.launches += 1


def _plain():
    return _Env(33, packed_step=True)


def _walking():
    return _Env(33)


def _po():
    return _Env(52, FRAME=26, obs_window=2)


def _normalised(venv, norm_obs=True):
    """DeviceVecNormalize around ``venv`` without its handle: what a wrapper outside it reads of it."""
    w = object.__new__(DeviceVecNormalize)
    DeviceVecEnvWrapper.__init__(w, venv, None)
    w.normalizer = SimpleNamespace(norm_obs=norm_obs, num_envs=N, obs_dim=venv.obs_dim)
    return w


@pytest.fixture
def recorders(monkeypatch):
    """Every layer class a wrapper's constructor creates raises _Reached: no refusal may come behind it."""
    def reached(*args, **kwargs):
        raise _Reached
    monkeypatch.setattr(normalize, "RunningNormalizer", reached)
    monkeypatch.setattr(perturb, "Perturbation", reached)
    monkeypatch.setattr(gait, "GaitReward", reached)


def test_the_chain_walk():
    from quadruped_gym_amd.envs.device_wrapper import base_env, stack_layer, stack_layers
    env = _walking()
    inner = DevicePrivilegedVecEnv(env, 1.0)
    outer = _normalised(inner)
    assert list(stack_layers(outer)) == [outer, inner] and list(stack_layers(env)) == [] and base_env(outer) is env and base_env(env) is env
    assert stack_layer(outer, "privileged") is inner and stack_layer(outer, "normalizer") is outer and stack_layer(inner, "normalizer") is None
    assert outer.obs_dim == 118 and outer.actor_obs_dim == 33 and getattr(env, "actor_obs_dim", None) is None


def test_normaliser_around_the_privileged_plain_env_is_refused(recorders):
    env = _plain()
    wide = DevicePrivilegedVecEnv(env, 1.0)
    assert wide.packed_step and wide.obs_dim == 118
    with pytest.raises(ValueError, match=r"DevicePrivilegedVecEnv\(DeviceVecNormalize\(env\)\)"):
        DeviceVecNormalize(wide)
    # ... through further wrappers too
    with pytest.raises(ValueError, match=r"DevicePrivilegedVecEnv\(DeviceVecNormalize\(env\)\)"):
        DeviceVecNormalize(_passthrough(wide))
    assert env.handles == ["privileged"]
    # the orders that work reach the handle: around the plain env itself, around the walking envs' wide rows
    for venv in (_plain(), DevicePrivilegedVecEnv(_walking(), 1.0), DevicePrivilegedVecEnv(_po(), 1.0)):
        with pytest.raises(_Reached):
            DeviceVecNormalize(venv)


def _passthrough(venv):
    """A wrapper with nothing of its own around ``venv``."""
    return DeviceVecEnvWrapper(venv, None)


def test_perturbation_around_the_privileged_wrapper_is_refused(recorders):
    for make in (_plain, _walking, _po):
        env = make()
        for venv in (DevicePrivilegedVecEnv(env, 1.0), _passthrough(DevicePrivilegedVecEnv(make(), 1.0))):
            with pytest.raises(ValueError, match=r"DevicePrivilegedVecEnv\(DevicePerturbedVecEnv\(env\)\)"):
                DevicePerturbedVecEnv(venv, obs_noise=0.1)
        assert env.handles == ["privileged"]
        with pytest.raises(_Reached):                           # next to the env, and around a normaliser: as ever
            DevicePerturbedVecEnv(make(), obs_noise=0.1)
        with pytest.raises(_Reached):
            DevicePerturbedVecEnv(_normalised(make()), obs_noise=0.1)


def test_command_gate_around_an_observation_normaliser_is_refused(recorders):
    env = _po()
    for venv in (_normalised(env), _passthrough(_normalised(env)), DevicePrivilegedVecEnv(_normalised(env), 1.0)):
        with pytest.raises(ValueError, match=r"DeviceVecNormalize\(DeviceGaitRewardVecEnv\(env, gate_on_command=True\)\)"):
            DeviceGaitRewardVecEnv(venv, gate_on_command=True)
    assert env.handles == ["privileged"]                        # the fixture's own; no contact sensor was asked for
    for venv in (_po(), _normalised(_po(), norm_obs=False), DevicePrivilegedVecEnv(_po(), 1.0)):
        with pytest.raises(_Reached):
            DeviceGaitRewardVecEnv(venv, gate_on_command=True)
    with pytest.raises(_Reached):                               # without the gate the order is free
        DeviceGaitRewardVecEnv(_normalised(_po()))
    with pytest.raises(ValueError, match="only the partially observable env"):
        DeviceGaitRewardVecEnv(_normalised(_walking()), gate_on_command=True)


def _unbound_normaliser(venv, obs_dim, terminal_dim):
    """DeviceVecNormalize around ``venv`` whose normaliser has no handle: every check ahead of the library can be reached."""
    nz = object.__new__(RunningNormalizer)
    nz.device, nz.num_envs, nz.obs_dim, nz._h, nz._lib = 0, N, obs_dim, None, None
    w = object.__new__(DeviceVecNormalize)
    DeviceVecEnvWrapper.__init__(w, venv, nz)
    w.normalizer, w.terminal_dim = nz, terminal_dim
    w._term_wide = object() if terminal_dim < obs_dim else None
    return w


def test_a_terminal_buffer_of_another_width_is_refused_before_the_envs_launch():
    import torch
    env = _po()
    w = _unbound_normaliser(DevicePrivilegedVecEnv(env, 1.0), 137, 52)
    z = lambda *shape: torch.zeros(shape)
    with pytest.raises(ValueError, match=r"\(8, 52\).*actor's width.*\(8, 137\)"):
        w.step_tensor(z(N, 12), z(N, 137), z(N), z(N), terminal_obs=z(N, 85))
    with pytest.raises(ValueError, match="actor's width"):
        w.step_tensor(z(N, 12), z(N, 137), z(N), z(N), terminal_obs=z(N + 1, 52))
    # the two widths it takes get as far as the device check of the tensor (these live on the host), still ahead of the launch
    for width in (52, 137):
        with pytest.raises(ValueError, match="terminal_obs must live on cuda:0"):
            w.step_tensor(z(N, 12), z(N, 137), z(N), z(N), terminal_obs=z(N, width))
    with pytest.raises(ValueError, match="obs must live on cuda:0"):
        w.step_tensor(z(N, 12), z(N, 137), z(N), z(N))
    # a stack without narrow terminal rows takes obs_dim columns only
    plain = _unbound_normaliser(_po(), 52, 52)
    with pytest.raises(ValueError, match="terminal_obs"):
        plain.step_tensor(z(N, 12), z(N, 52), z(N), z(N), terminal_obs=z(N, 26))
    assert env.launches == 0 and plain.venv.launches == 0
