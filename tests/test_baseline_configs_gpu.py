"""BASELINE.json configs 3 and 4 at their real sizes, through the C ABI.

config 3: 32 768 envs on one MI355X, randomized initial heading (QG_RESET_RANDOM_YAW, walking_quad.py:68-75) -- AUTO picks the
          two-legs-per-lane kernel there; a strided sample of the shard is compared with the oracle from identical states, the
          whole shard through size-independent invariants over > 100 env-steps including auto-resets.
config 4: 262 144 envs = 8 x 32 768; the total batch on ONE GPU through the invariants, and rank r's shard (env_index_base =
          r * 32 768) bit for bit against the same rows of the whole batch -- sharding must not change results.
The one-step tolerances are the ones stated in tests/parity.py (f32 kernel vs f64 oracle).
"""
import numpy as np
import pytest

from quadruped_gym_amd import _abi
from parity import TOL, close

pytestmark = pytest.mark.gpu

CTRL_RANGE = np.array([0.5, 0.91, 1.0] * 4)


def _task(max_time, fall=False):
    t = _abi.default_task()
    t.max_time = max_time
    t.auto_reset = 1
    t.reset_flags = _abi.RESET_RANDOM_YAW
    if fall:
        t.use_fall, t.fall_height = 1, 0.05
    return t


def _invariants(qpos, qvel, act):
    assert np.isfinite(qpos).all() and np.isfinite(qvel).all() and np.isfinite(act).all()
    assert np.abs(np.linalg.norm(qpos[:, 3:7], axis=1) - 1.0).max() < 1e-5            # unit quaternions
    assert qpos[:, 2].min() > 0.0 and qpos[:, 2].max() < 0.3 and np.abs(qvel).max() < 100.0
    assert (np.abs(act) <= CTRL_RANGE + 1e-6).all()                                   # activations inside the ctrlrange


def test_config3_32768_envs_random_yaw_sample_against_oracle(oracle):
    import torch
    from quadruped_gym_amd.sim import BatchedSim
    n, seed, base = 32768, 2025, 7 * 32768
    task = _task(max_time=0.6, fall=True)                   # 300 substeps: every env restarts at env-step 75 (or earlier if it falls)
    sim = BatchedSim(n, task=task, env_index_base=base)
    assert sim.mapping == _abi.MAP_PAIR                     # AUTO: the production kernel of this batch size
    sim.reset(seed=seed, flags=_abi.RESET_RANDOM_YAW)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev); gen.manual_seed(5)
    pool = [torch.rand((n, 12), generator=gen, device=dev) * 2.4 - 1.2 for _ in range(8)]     # some beyond the +-1 clip
    packed = torch.empty((n, 35), device=dev)
    episodes = np.zeros(n, np.int64)
    total_done = 0
    for k in range(130):
        sim.step_device_packed(pool[k % 8], packed)
        d = packed[:, 34].cpu().numpy() > 0.5
        episodes += d
        total_done += int(d.sum())
        if k == 74:
            # the time limit has just ended every episode still running: the whole shard stands at its randomized start pose,
            # heading drawn from each env's own (seed, global env index, episode) stream
            assert d.sum() > 0.9 * n
            qpos, qvel, act, _, nstep = sim.get_state()
            assert not nstep[d].any() and not qvel[d].any() and not act[d].any()
            for i in np.nonzero(d)[0][::97]:
                a = 2 * np.pi * oracle.uniform(seed, base + int(i), int(episodes[i]))
                assert np.allclose(qpos[i, 3:7], [np.cos(a / 2), 0, 0, np.sin(a / 2)], atol=2e-7), i
                assert np.array_equal(qpos[i, [0, 1, 2]], np.array(sim.model.qpos0[:3], np.float32))
            yaw = 2 * np.arctan2(qpos[d, 6], qpos[d, 3])
            assert np.ptp(yaw) > 6.0                          # the headings really spread over the circle
    assert total_done >= n                                    # every env went through at least one auto-reset
    qpos, qvel, act, _, nstep = sim.get_state()
    _invariants(qpos, qvel, act)
    assert nstep.max() <= 300 and (nstep % 4 == 0).all()

    # ---- one more env-step of the whole shard; 512 envs spread over it against the oracle from the same f32 states -------------
    idx = np.arange(0, n, 64) + (np.arange(n // 64) % 64)     # every lane position of the 32-env waves, every 64th env
    assert len(idx) == 512
    actions = pool[3].cpu().numpy()
    otask = oracle.default_task()
    otask.max_time, otask.use_fall, otask.fall_height = 0.6, 1, 0.05
    b = oracle.Batch(oracle.default_model(), otask, len(idx))
    b.set_state(qpos[idx].astype(np.float64), qvel[idx].astype(np.float64), act[idx].astype(np.float64), None, nstep[idx])
    obs_o, rew_o, done_o, _ = b.step(actions[idx].astype(np.float64))
    q_o, v_o, a_o, _, n_o = b.get_state()
    sim.step_device_packed(pool[3], packed)
    p = packed.cpu().numpy()[idx]
    q1, v1, a1, _, n1 = [x[idx] for x in sim.get_state()]
    t = TOL["A"]
    mask = np.ones(33, bool); mask[12:15] = False
    close(p[:, :33][:, mask], obs_o[:, mask], t["obs"], "obs")
    close(p[:, 12:15], obs_o[:, 12:15], t["accel"], "accelerometer")
    close(p[:, 33], rew_o, t["reward"], "reward")
    sure = np.abs(q_o[:, 2] - 0.05) > 1e-4
    assert np.array_equal(p[sure, 34] > 0.5, done_o[sure])
    run = ~(p[:, 34] > 0.5) & sure                            # envs that did not finish: the integrated state
    assert run.sum() > 400
    close(q1[run], q_o[run], t["qpos"], "qpos")
    close(v1[run], v_o[run], t["qvel"], "qvel")
    close(a1[run], a_o[run], t["act"], "act")
    assert np.array_equal(n1[run], n_o[run])
    sim.close()


def test_config4_262144_envs_invariants_and_shard_equivalence(oracle):
    import torch
    from quadruped_gym_amd.sim import BatchedSim
    n_total, n_shard, seed = 262144, 32768, 99
    task = _task(max_time=0.2)                              # 100 substeps -> every env restarts at env-step 25
    whole = BatchedSim(n_total, task=task)
    assert whole.mapping == _abi.MAP_PAIR
    ranks = (0, 5)                                           # two of the eight shards of the driver's config-4 run
    shards = {r: BatchedSim(n_shard, task=task, env_index_base=r * n_shard) for r in ranks}
    for s in [whole] + list(shards.values()):
        s.reset(seed=seed, flags=_abi.RESET_RANDOM_YAW)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev); gen.manual_seed(11)
    pool = [torch.rand((n_total, 12), generator=gen, device=dev) * 2 - 1 for _ in range(4)]
    packed = torch.empty((n_total, 35), device=dev)
    spacked = {r: torch.empty((n_shard, 35), device=dev) for r in ranks}
    for k in range(110):
        whole.step_device_packed(pool[k % 4], packed)
        for r in ranks:
            sl = slice(r * n_shard, (r + 1) * n_shard)
            shards[r].step_device_packed(pool[k % 4][sl].contiguous(), spacked[r])
            if k % 10 == 4 or k in (24, 25, 49):             # includes the steps that auto-reset and the first ones after
                assert torch.equal(packed[sl], spacked[r]), (k, r)
        if k == 24:
            d = packed[:, 34].cpu().numpy()
            assert (d == 1.0).all()                            # the f64-accumulated clock crosses 0.2 s at substep 100 in every env
            qpos = whole.get_state()[0]
            for i in range(0, n_total, 4099):
                a = 2 * np.pi * oracle.uniform(seed, i, 1)     # second draw of env i's stream (the explicit reset took counter 0)
                assert np.allclose(qpos[i, 3:7], [np.cos(a / 2), 0, 0, np.sin(a / 2)], atol=2e-7), i
    torch.cuda.synchronize()
    qpos, qvel, act, _, nstep = whole.get_state()
    _invariants(qpos, qvel, act)
    assert (nstep == 4 * (110 % 25)).all()
    for r in ranks:                                          # the shard's state equals its rows of the whole batch, bit for bit
        sq, sv, sa, _, sn = shards[r].get_state()
        sl = slice(r * n_shard, (r + 1) * n_shard)
        assert np.array_equal(sq, qpos[sl]) and np.array_equal(sv, qvel[sl]) and np.array_equal(sa, act[sl]) and np.array_equal(sn, nstep[sl])
    for s in [whole] + list(shards.values()):
        s.close()
