"""The two device-side VecEnv wrappers stacked, and the plain env's own snapshot.  A perturbation layer with every standard deviation
and the latency at zero is the identity on bits, so DeviceVecNormalize(DevicePerturbedVecEnv(env)) must step, checkpoint, resume and
close like DeviceVecNormalize(twin) -- through both wrappers' pass-through, buffer binding, snapshot and close.  64 envs whose
episodes end inside ten steps (max_time 0.05 s).  Default stream, no capture."""
import numpy as np
import pytest
import torch

from quadruped_gym_amd.envs.vec_env import QuadrupedVecEnv
from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
from quadruped_gym_amd.normalize import DeviceVecNormalize
from quadruped_gym_amd.perturb import DevicePerturbedVecEnv

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N = 64
PLAIN = dict(reward_fns={"forward": 1.0, "control_cost": -0.1, "alive_bonus": 1.0}, termination_fns={"fall": 0.05}, max_time=0.05)
PO = dict(random_controls=True, random_init=True, device_commands=True, reset_options={"min_speed": 0.0, "max_speed": 0.5}, max_time=0.05,
          nan_direction=False, obs_window=3)


def _bits(*tensors):
    torch.cuda.synchronize()
    return b"".join(t.cpu().numpy().tobytes() for t in tensors)


def _norm_bytes(wrapper):
    sd = wrapper.normalizer.state_dict()
    return b"".join(np.asarray(sd[k]).tobytes() for k in sorted(sd))


def _actions(steps):
    gen = torch.Generator(device=DEV).manual_seed(11)
    return torch.rand((steps, N, 12), generator=gen, device=DEV) * 2 - 1


def _step(wrapper, kind, actions):
    """One step_tensor; (the bits of everything it filled, the number of finished envs)."""
    if kind == "plain":
        packed = wrapper.step_tensor(actions)
        return _bits(packed), int((packed[:, -1] != 0).sum())
    D = wrapper.obs_dim
    obs, term = torch.zeros((N, D), device=DEV), torch.zeros((N, D), device=DEV)
    rew, done = torch.zeros(N, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV)
    assert wrapper.step_tensor(actions, obs, rew, done, terminal_obs=term) is None
    return _bits(obs, rew, done, term), int(done.sum())


@pytest.mark.parametrize("kind", ["plain", "po"])
def test_a_silent_perturbation_under_the_normaliser_is_the_identity(kind):
    make = (lambda: QuadrupedVecEnv(N, **PLAIN)) if kind == "plain" else (lambda: POWalkingQuadrupedVecEnv(N, **PO))
    env, twin = make(), make()
    inner = DevicePerturbedVecEnv(env, seed=3)
    stack, ref = DeviceVecNormalize(inner), DeviceVecNormalize(twin)
    assert stack.venv is inner and inner.venv is env and stack.num_envs == N and stack.obs_dim == env.obs_dim == stack.normalizer.obs_dim
    assert inner.perturbation.delay_range == (0, 0)
    acts = _actions(10)
    assert np.array_equal(stack.reset().view(np.uint32), ref.reset().view(np.uint32))
    finished = 0
    for k in range(4):
        a = acts[k].clone()
        got, fin = _step(stack, kind, a)
        assert got == _step(ref, kind, acts[k])[0] and torch.equal(a, acts[k]), k
        assert _norm_bytes(stack) == _norm_bytes(ref), k
        finished += fin
    snap = stack.snapshot()
    assert set(snap) == {"env", "normalizer", "training"} and set(snap["env"]) == {"env", "perturbation"} and "sim" in snap["env"]["env"]
    first = []
    for k in range(4, 7):
        got, fin = _step(stack, kind, acts[k])
        assert got == _step(ref, kind, acts[k])[0] and _norm_bytes(stack) == _norm_bytes(ref), k
        first.append((got, _norm_bytes(stack)))
        finished += fin
    stack.restore(snap)
    assert [(_step(stack, kind, acts[k])[0], _norm_bytes(stack)) for k in range(4, 7)] == first
    for k in range(7, 10):
        got, fin = _step(stack, kind, acts[k])
        assert got == _step(ref, kind, acts[k])[0] and _norm_bytes(stack) == _norm_bytes(ref), k
        finished += fin
    assert finished >= N                                            # every env's episode ended at least once on the way
    stack.close()
    assert stack.normalizer._h is None and inner.perturbation._h is None and env._sim is None
    ref.close()


def test_the_plain_env_snapshot_carries_the_contact_timers():
    env = QuadrupedVecEnv(N, **PLAIN)
    sensor = env.contact_sensor()
    D = env.obs_dim
    acts = _actions(10)
    env.reset()

    def rounds(lo, hi):
        out = []
        for k in range(lo, hi):
            packed = env.step_tensor(acts[k])
            _, feet = sensor.read(done=packed[:, D + 1])
            out.append((_bits(feet), sensor.state().tobytes()))
        return out

    rounds(0, 4)
    snap = env.snapshot()
    assert set(snap) == {"sim", "contact"} and np.array_equal(snap["contact"], sensor.state())
    first = rounds(4, 7)
    assert first[-1][1] != snap["contact"].tobytes()                # the timers moved on
    env.restore(snap)
    assert rounds(4, 7) == first
    # a wrapper's snapshot holds the env's, timers included
    wrapped = DeviceVecNormalize(env)
    assert set(wrapped.snapshot()["env"]) == {"sim", "contact"}
    # all or nothing: a snapshot without timers is refused before anything is written
    before = env._sim.get_state()
    timers = sensor.state()
    with pytest.raises(ValueError, match="no contact-sensor timers"):
        env.restore({"sim": snap["sim"]})
    assert all(np.array_equal(x, y) for x, y in zip(before, env._sim.get_state())) and np.array_equal(timers, sensor.state())
    assert not np.array_equal(before[0], snap["sim"]["qpos"])      # (the refused snapshot would have changed it)
    wrapped.close()
    assert env._sim is None and sensor._h is None
