"""The walking envs on their handle classes (quadruped_gym_amd/task_layers.py): ``step_tensor`` refuses every tensor the library
would have written out of bounds BEFORE anything is launched, the layers die with (and before) their simulator whoever closes what,
and an env that is dropped without ``close()`` gives its device memory back."""
import gc

import numpy as np
import pytest
import torch

from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv, WalkingQuadrupedVecEnv

pytestmark = pytest.mark.gpu

N, WINDOW = 3, 2
MIB = 1 << 20


def _make(kind, n=N):
    kw = dict(max_time=0.024, random_init=True, random_controls=True, device_commands=True, seed=5)     # episodes of three env-steps
    return WalkingQuadrupedVecEnv(n, **kw) if kind == "walking" else POWalkingQuadrupedVecEnv(n, obs_window=WINDOW, **kw)


def _buffers(env):
    dev = torch.device("cuda", env.device)
    n, D = env.num_envs, env.obs_dim
    bufs = dict(obs=torch.zeros((n, D), device=dev), reward=torch.zeros(n, device=dev), done=torch.zeros(n, dtype=torch.uint8, device=dev),
                components=torch.zeros((n, 11), device=dev))
    if isinstance(env, POWalkingQuadrupedVecEnv):
        bufs["terminal_obs"] = torch.zeros((n, D), device=dev)
    return bufs


def _bits(bufs):
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().tobytes() for k, t in bufs.items()}


def _fingerprint(env):
    """Everything a launch would have moved: physics state and step counters, commands, the estimator."""
    arrays = list(env._sim.get_state()) + list(env.commands()) + list(env.estimates())
    return [np.array(a).tobytes() for a in arrays]


@pytest.mark.parametrize("kind", ["walking", "po"])
def test_step_tensor_refuses_bad_tensors_before_any_launch(kind):
    env, twin = _make(kind), _make(kind)
    dev = torch.device("cuda", env.device)
    D = env.obs_dim
    assert D == (33 if kind == "walking" else 26 * WINDOW) and not env.packed_step
    gen = torch.Generator().manual_seed(0)
    acts = [(torch.rand((N, 12), generator=gen) * 2 - 1).to(dev) for _ in range(3)]
    good, twin_bufs = _buffers(env), _buffers(twin)
    for e, b in ((env, good), (twin, twin_bufs)):
        e.reset()
        e.step_tensor(acts[0], **b)
    assert _bits(good) == _bits(twin_bufs)

    f32 = dict(dtype=torch.float32, device=dev)
    bad = {"obs as float64": dict(obs=torch.zeros((N, D), dtype=torch.float64, device=dev)),
           "obs with 4 rows": dict(obs=torch.zeros((4, D), **f32)),
           "obs transposed": dict(obs=torch.zeros((D, N), **f32).t()),
           "actions on the CPU": dict(actions=acts[1].cpu()),
           "reward of shape (3, 1)": dict(reward=torch.zeros((N, 1), **f32)),
           "done as int32": dict(done=torch.zeros(N, dtype=torch.int32, device=dev)),
           "components of width 10": dict(components=torch.zeros((N, 10), **f32))}
    if kind == "po":
        bad["terminal_obs one short"] = dict(terminal_obs=torch.zeros((N, D - 1), **f32))
    before, rows = _fingerprint(env), _bits(good)
    for what, swap in bad.items():
        args = dict(good, actions=acts[1])
        args.update(swap)
        with pytest.raises(ValueError):
            env.step_tensor(**args)
        assert _fingerprint(env) == before, what
        assert _bits(good) == rows, what

    # bool is one byte as uint8 is: accepted, and the same bits as the twin that was given uint8 and never saw a bad call
    as_bool = dict(good, done=torch.zeros(N, dtype=torch.bool, device=dev))
    env.step_tensor(acts[1], **as_bool)
    twin.step_tensor(acts[1], **twin_bufs)
    assert _bits(as_bool) == _bits(twin_bufs)
    env.step_tensor(acts[2], **good)                        # the third env-step ends every episode: terminal stacks included
    twin.step_tensor(acts[2], **twin_bufs)
    assert _bits(good) == _bits(twin_bufs)
    assert good["done"].any()
    assert _fingerprint(env) == _fingerprint(twin)
    env.close()
    twin.close()


def test_closing_the_simulator_first_closes_the_layers_before_it():
    env = POWalkingQuadrupedVecEnv(2, obs_window=WINDOW)
    env.reset()
    sim, walk, pack = env._sim, env._walk, env._obs_pack
    env._sim.close()
    assert sim._h is None and walk._h is None and pack._h is None
    env.close()
    env.close()
    fresh = POWalkingQuadrupedVecEnv(2, obs_window=WINDOW)
    fresh.reset()
    obs, rew, done, infos = fresh.step(np.zeros((2, 12), np.float32))
    assert obs.shape == (2, 26 * WINDOW) and np.isfinite(obs).all() and len(infos) == 2
    fresh.close()


def test_envs_dropped_without_close_return_their_device_memory():
    """One cycle: create, reset, one step, drop -- never ``close()``.  A 256-env pack of window 10 with its walking layer and simulator
    holds a few MiB, so a layer left behind per cycle shows within a few of the thirty cycles.  Measured on an MI355X: 0 bytes taken;
    the parent commit, whose env kept the two layers as bare pointers without a ``__del__``, took 202 MiB (6.7 MiB per cycle)."""
    acts = np.zeros((256, 12), np.float32)

    def cycle():
        env = POWalkingQuadrupedVecEnv(256, obs_window=10)
        env.reset()
        env.step(acts)
        del env
        gc.collect()

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    for _ in range(3):
        cycle()
    start = free()
    for _ in range(30):
        cycle()
    end = free()
    print(f"free device memory before and after thirty dropped envs: {start} {end} ({(start - end) / MIB:.2f} MiB taken)")
    assert abs(start - end) <= MIB
