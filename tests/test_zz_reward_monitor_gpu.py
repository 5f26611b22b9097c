"""The reward monitor on the GPU (qg_monitor_*, csrc/qg_monitor.hip) against the float64 definition of tests/reward_monitor_reference.py:
log rows within MARGIN x the measured budget and the per-env accumulators bit for bit at every shape on either side of the
partition's boundaries, strided inputs and the three done types with the contiguous call's bits, the ring's order, graph replay and
the state's round trip bit for bit, the rollout buffer's episode statistics, a walking env end to end, and nothing written but the
row.  With QG_MONITOR_PARITY_OUT=<file> the parity cases append their largest error as a share of the bound (profiles/r26).
The module's name puts it last in collection, as the other modules that capture hipGraphs on a side stream.

Bounds.  A mean: MARGIN x BUDGET_MEAN x eps64 x mean|x|; the std: MARGIN x BUDGET_STD x eps64 x (std + |mean|); the totals: the
mean's bound as a sum's, MARGIN x BUDGET_MEAN x eps64 x (the magnitudes of everything folded so far) -- the error of a sum relative
to the sum of the magnitudes is the unit the budget was measured in."""
import os

import numpy as np
import pytest
import torch

import reward_monitor_reference as R

from quadruped_gym_amd.monitor import RewardMonitor

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _record(line):
    print(line)
    out = os.environ.get("QG_MONITOR_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def _keys(C):
    return ["term%d" % c for c in range(C)]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                    # (a copy: the shared inputs are read-only)


def _device_inputs(n, C):
    comps, reward, done = R.inputs(n, C)
    return _dev(comps), _dev(reward), _dev(done.astype(np.uint8))


def _bits(mon):
    """Everything a monitor holds, as integers: the ring, the accumulators, the totals and the counters."""
    s = mon.state()
    return np.concatenate([s["log"].view(np.uint64).ravel(), s["acc"].view(np.uint64).ravel(), s["len"].astype(np.uint64),
                           s["totals"].view(np.uint64), np.array([s["episodes"], s["length_sum"], s["records"]], np.uint64)])


# ---- 1. parity at every shape ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C", R.shapes())
def test_rows_accumulators_and_totals_are_the_reference(n, C):
    comps, reward, done = R.inputs(n, C)
    d_comps, d_reward, d_done = _device_inputs(n, C)
    want = R.replay(n, C)
    mon = RewardMonitor(n, _keys(C), capacity=R.STEPS)
    quiet = {}
    for t in range(R.STEPS):
        if t in R.NOBODY:
            quiet[t] = mon.episode_stats(clear=False)
        mon.record(d_comps[t], d_reward[t], d_done[t])
        if t in R.NOBODY:                                                           # nobody finished: the totals bit for bit
            after = mon.episode_stats(clear=False)
            assert np.array_equal(after["totals"].view(np.uint64), quiet[t]["totals"].view(np.uint64))
            assert (after["episodes"], after["length_sum"]) == (quiet[t]["episodes"], quiet[t]["length_sum"])
    s = mon.state()
    mon.close()
    log = s["log"]
    share_mean = share_std = 0.0
    for t in range(R.STEPS):
        tol = R.row_tolerance(comps[t], reward[t])
        err = np.abs(log[t] - want.log[t])
        share_mean = max(share_mean, float((err[:C + 1] / tol[:C + 1]).max()))
        share_std = max(share_std, float(err[C + 1] / tol[C + 1]) if tol[C + 1] > 0 else float(err[C + 1] > 0))
        assert log[t, C + 2] == done[t].sum()                                       # exact
    tol_totals = want.totals_tolerance()
    share_totals = float((np.abs(s["totals"] - want.totals) / tol_totals).max())
    _record("n %6d C %2d: largest share of the bound: means %.3f, std %.3f, totals %.3f" % (n, C, share_mean, share_std, share_totals))
    assert share_mean <= 1.0 and share_std <= 1.0 and share_totals <= 1.0
    if n == 1:
        assert not log[:, C + 1].any()                                              # one env: the std is exactly 0
    assert np.array_equal(s["acc"].view(np.uint64), want.acc.view(np.uint64))       # one IEEE add per step: these bits
    assert np.array_equal(s["len"], want.len)
    assert (s["episodes"], s["length_sum"], s["records"]) == (want.episodes, want.length_sum, R.STEPS)
    assert want.episodes >= n + 1                                                   # the script: everybody once, one env, the random rest


def test_constant_reward_has_zero_std_and_every_env_finishing_folds_everything():
    n, C = 2 * R.implementation_constants()["TILE"] + 37, 3
    d_comps, _, _ = _device_inputs(n, C)
    reward = torch.full((n,), 0.1, device=DEV)
    everybody = torch.ones(n, device=DEV, dtype=torch.uint8)
    mon = RewardMonitor(n, _keys(C), capacity=4)
    mon.record(d_comps[0], reward)                                                  # done=None: nobody finished
    mon.record(d_comps[1], reward, everybody)
    s = mon.state()
    mon.close()
    assert s["log"][0, C + 1] == 0.0 and s["log"][1, C + 1] == 0.0
    assert np.array_equal(s["log"][:2, C], np.full(2, np.float64(np.float32(0.1))))
    assert list(s["log"][:2, C + 2]) == [0.0, float(n)]
    assert not s["acc"].any() and not s["len"].any() and (s["episodes"], s["length_sum"]) == (n, 2 * n)
    assert abs(s["totals"][C] - 2 * n * np.float64(np.float32(0.1))) <= R.MARGIN * R.BUDGET_MEAN * R.EPS * 2 * n * 0.1


# ---- 2. strides, alignment and the done types ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [11, 32])
def test_strided_inputs_give_the_contiguous_bits(C):
    n = 65
    comps, reward, done = R.inputs(n, C)
    plain = RewardMonitor(n, _keys(C), capacity=R.STEPS)
    d_comps, d_reward, d_done = _device_inputs(n, C)
    for t in range(R.STEPS):
        plain.record(d_comps[t], d_reward[t], d_done[t])
    want = _bits(plain)
    plain.close()
    wide = torch.zeros((n, C + 8), device=DEV)                                      # the terms at columns 3 .. 3 + C: rows 4-byte aligned only
    packed = torch.zeros((n, 35), device=DEV)                                       # the plain env's rows: reward and done are columns 33, 34
    for kind in ("f32 column", "uint8", "bool"):
        mon = RewardMonitor(n, _keys(C), capacity=R.STEPS)
        for t in range(R.STEPS):
            wide[:, 3:3 + C] = d_comps[t]
            packed[:, 33], packed[:, 34] = d_reward[t], d_done[t].float()
            d = {"f32 column": packed[:, 34], "uint8": d_done[t], "bool": d_done[t].bool()}[kind]
            mon.record(wide[:, 3:3 + C], packed[:, 33], d)
        assert np.array_equal(_bits(mon), want), kind
        mon.close()


# ---- 3. the ring --------------------------------------------------------------------------------------------------------------------
def test_ring_is_chronological_and_the_csv_is_the_references(tmp_path):
    n, C = 64, 11
    from quadruped_gym_amd.envs.walking import REWARD_KEYS
    comps, reward, done = R.inputs(n, C)
    d_comps, d_reward, d_done = _device_inputs(n, C)
    mon = RewardMonitor(n, REWARD_KEYS, capacity=4)
    assert mon.rows()["step"].size == 0
    for t in range(10):
        mon.record(d_comps[t], d_reward[t], d_done[t])
    rows = mon.rows()
    assert list(rows["step"]) == [6, 7, 8, 9] and mon.records == 10
    assert list(rows) == ["step"] + REWARD_KEYS + ["reward", "std", "dones"]
    for j, t in enumerate(range(6, 10)):
        want, tol = R.log_row(comps[t], reward[t], done[t]), R.row_tolerance(comps[t], reward[t])
        got = np.array([rows[k][j] for k in REWARD_KEYS + ["reward", "std", "dones"]])
        assert (np.abs(got - want) <= tol).all(), t
    path = tmp_path / "rewards_continuous.csv"
    mon.to_csv(path)
    assert open(path, newline="").read() == R.csv_text(REWARD_KEYS, rows)
    mon.reset(clear_log=True)
    assert mon.records == 0 and mon.rows()["step"].size == 0 and not mon.log.any()
    mon.close()


def test_only_the_row_is_written():
    n, C = 65, 3
    d_comps, d_reward, d_done = _device_inputs(n, C)
    keep = [x.clone() for x in (d_comps, d_reward, d_done)]
    mon = RewardMonitor(n, _keys(C), capacity=8)
    sentinel = -12345.678
    for t in range(3):
        mon.log.fill_(sentinel)
        mon.record(d_comps[t], d_reward[t], d_done[t])
        log = mon.state()["log"]
        assert (np.delete(log, t, axis=0) == sentinel).all() and (log[t] != sentinel).all()
    assert all(torch.equal(a, b) for a, b in zip(keep, (d_comps, d_reward, d_done)))
    mon.close()


# ---- 4. graph replay, state ---------------------------------------------------------------------------------------------------------
def test_graph_replay_is_the_eager_run():
    """One record captured on a side stream and replayed 8 times, the inputs rewritten between replays: the bits of 8 eager calls."""
    n, C = 2 * R.implementation_constants()["TILE"] + 37, 11
    d_comps, d_reward, d_done = _device_inputs(n, C)
    eager, mon = RewardMonitor(n, _keys(C), capacity=6), RewardMonitor(n, _keys(C), capacity=6)
    for t in range(8):
        eager.record(d_comps[t], d_reward[t], d_done[t])
    s_comps, s_reward, s_done = torch.zeros((n, C), device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV, dtype=torch.uint8)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        mon.record(s_comps, s_reward, s_done, stream=side)
    mon.reset(clear_totals=True, clear_log=True)                                    # whatever a capture may have run, start fresh
    for t in range(8):
        s_comps.copy_(d_comps[t]), s_reward.copy_(d_reward[t]), s_done.copy_(d_done[t])
        torch.cuda.synchronize()
        graph.replay()
    torch.cuda.synchronize()
    assert mon.records == 8                                                         # the cursor moved on the device
    assert np.array_equal(_bits(mon), _bits(eager))
    del graph
    mon.close(), eager.close()


def test_a_restored_monitor_continues_bit_for_bit():
    n, C = 257, 11
    d_comps, d_reward, d_done = _device_inputs(n, C)
    a = RewardMonitor(n, _keys(C), capacity=5)
    for t in range(8):
        a.record(d_comps[t], d_reward[t], d_done[t])
    state = a.state()
    b = RewardMonitor(n, _keys(C), capacity=5)
    b.load_state(state)
    assert np.array_equal(_bits(a), _bits(b))
    for t in range(8, 12):
        a.record(d_comps[t], d_reward[t], d_done[t]), b.record(d_comps[t], d_reward[t], d_done[t])
    assert np.array_equal(_bits(a), _bits(b))
    want = R.replay(n, C)
    assert np.array_equal(b.state()["acc"].view(np.uint64), want.acc.view(np.uint64)) and b.records == R.STEPS
    # a masked reset empties the named envs' running episodes and nothing else
    mask = np.arange(n) % 3 == 0
    before = b.state()
    b.reset(mask)
    after = b.state()
    assert not after["acc"][mask].any() and not after["len"][mask].any()
    assert np.array_equal(after["acc"][~mask], before["acc"][~mask]) and np.array_equal(after["len"][~mask], before["len"][~mask])
    assert np.array_equal(after["totals"], before["totals"]) and after["records"] == before["records"]
    stats = b.episode_stats(clear=True)
    assert stats["episodes"] == want.episodes and b.episode_stats()["episodes"] == 0 and np.isnan(b.episode_stats()["ep_rew_mean"])
    assert np.array_equal(b.state()["acc"], after["acc"])                           # clear keeps the running episodes
    a.close(), b.close()


# ---- 5. beside the other layers ---------------------------------------------------------------------------------------------------
def test_episode_statistics_are_the_rollout_buffers():
    """The same (reward, done) stream into a DeviceRolloutBuffer and the monitor: the same episodes and lengths; the reward's mean
    episode sum within the two summations' bounds (each side deviates from the exact sum by at most its own)."""
    from quadruped_gym_amd.rollout import DeviceRolloutBuffer
    n, C = 65, 3
    d_comps, d_reward, d_done = _device_inputs(n, C)
    want = R.replay(n, C)
    buf = DeviceRolloutBuffer(n, R.STEPS, 4, 2)
    mon = RewardMonitor(n, _keys(C), capacity=R.STEPS)
    obs, act, vec = torch.zeros((n, 4), device=DEV), torch.zeros((n, 2), device=DEV), torch.zeros(n, device=DEV)
    buf.begin(obs)
    for t in range(R.STEPS):
        buf.add(obs, act, vec, vec, d_reward[t], d_done[t])
        mon.record(d_comps[t], d_reward[t], d_done[t])
    theirs, ours = buf.episode_stats(), mon.episode_stats()
    buf.close(), mon.close()
    assert ours["episodes"] == theirs["episodes"] == want.episodes
    assert ours["ep_len_mean"] == theirs["ep_len_mean"] == want.length_sum / want.episodes
    tol = 2 * want.totals_tolerance()[C] / want.episodes
    _record("rollout buffer ep_rew_mean %.17g, monitor %.17g, bound %.3e" % (theirs["ep_rew_mean"], ours["ep_rew_mean"], tol))
    assert abs(ours["ep_rew_mean"] - theirs["ep_rew_mean"]) <= tol
    assert set(ours["terms"]) == set(_keys(C))
    assert abs(ours["terms"]["term0"] - want.totals[0] / want.episodes) <= want.totals_tolerance()[0] / want.episodes


def test_walking_env_end_to_end():
    """30 steps of the walking env with the monitor recording: the log's term means are the float64 means of the recorded components,
    and the terms add up to the reward to the float32 rounding of the kernel's own eleven-term sum."""
    from quadruped_gym_amd.envs.walking import WalkingQuadrupedVecEnv
    n, T = 64, 30
    env = WalkingQuadrupedVecEnv(n, max_time=0.1, device_commands=True, random_controls=True, nan_direction=False)
    env.reset()
    mon = RewardMonitor.for_env(env, capacity=T)
    assert mon.keys == list(env.reward_keys) and mon.num_envs == n and mon.n_terms == 11
    obs, rew = torch.zeros((n, 33), device=DEV), torch.zeros(n, device=DEV)
    done, comps = torch.zeros(n, device=DEV, dtype=torch.uint8), torch.zeros((n, 11), device=DEV)
    acts = _dev(np.random.default_rng(4).uniform(-1, 1, (T, n, 12)).astype(np.float32))
    seen = []
    for t in range(T):
        env.step_tensor(acts[t], obs, rew, done, components=comps)
        mon.record(comps, rew, done)
        seen.append((comps.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()))
    rows, stats = mon.rows(), mon.episode_stats()
    mon.close(), env.close()
    assert list(rows["step"]) == list(range(T)) and np.isfinite(np.stack([rows[k] for k in mon.keys])).all()
    share = 0.0
    for t, (c, r, d) in enumerate(seen):
        want, tol = R.log_row(c, r, d), R.row_tolerance(c, r)
        got = np.array([rows[k][t] for k in mon.keys + ["reward", "std", "dones"]])
        ok = tol > 0
        share = max(share, float((np.abs(got - want)[ok] / tol[ok]).max()))
        assert (np.abs(got - want) <= tol).all(), t
        # the kernel adds the eleven terms in float32: per env at most 11 roundings of at most half an ulp of the running magnitude
        f32_sum = 11 * 2.0 ** -24 * np.abs(c.astype(np.float64)).sum(1).mean()
        assert abs(got[:11].sum() - got[11]) <= f32_sum + tol[:12].sum(), t
    _record("walking env, 30 steps of 64 envs: largest share of the bound %.3f; episodes %d" % (share, stats["episodes"]))
    finished = sum(int(d.sum()) for _, _, d in seen)
    assert stats["episodes"] == finished >= n and stats["ep_len_mean"] > 1 and set(stats["terms"]) == set(mon.keys)
