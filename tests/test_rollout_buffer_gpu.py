"""The rollout buffer on the GPU (qg_rollout_*, csrc/qg_rollout.hip) against the float64 checker of tests/rollout_buffer_reference.py.

Stored rows, gathered rows and everything under graph replay are compared bit for bit.  A reward with a truncation bootstrap is within
one float32 ulp of f32(r + f32(gamma) tv).  GAE: |A - A64| and |returns - R64| <= 8 * 2^-24 * M * S with
M = max|r| + (1 + gamma) max|v| + gamma lambda max|A64| and S = sum_{j<F} (gamma lambda)^j: at most eight roundings per step, each
relative to a term bounded by M, carried on by the recurrence with the factor gamma lambda.  A NumPy float32 loop in the header's order
reaches 0.33 of that bound on these input families (tests/test_rollout_buffer_api.py).  The device, measured on an MI355X over all
the cases below (profiles/r14/rollout_buffer_parity.txt): 0.53 at K = 1, n = 1 (one env whose last value, 6.0, enters the sum while M counts
its one stored value, 0.16), 0.12 or less on every other shape; an indexing or masking error is larger by orders of magnitude.
With QG_ROLLOUT_PARITY_OUT=<file> every GAE case appends its largest ratio to that file."""
import functools
import os

import numpy as np
import pytest
import torch

import rollout_buffer_reference as R
from policy_checks import DEV

from quadruped_gym_amd.rollout import DeviceRolloutBuffer, RolloutBufferSamples

pytestmark = pytest.mark.gpu
IDS = ["x".join(str(v) for v in s) for s in R.SHAPES]
STORED = ("observations", "actions", "log_probs", "values", "rewards", "dones", "advantages", "returns")


def _record(line):
    print(line)
    out = os.environ.get("QG_ROLLOUT_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _steps(K, n, D, A):
    """The rows of K + 2 env-steps (float32 / uint8 NumPy, never modified): obs0, then per step next_obs, actions, log_prob, value,
    reward, done (20 %), trunc_value (where done, half of them), episode_reward."""
    rng = np.random.default_rng([K, n, D, A])
    T = K + 2
    f = np.float32
    done = (rng.random((T, n)) < 0.2).astype(np.uint8)
    trunc = (3.0 * rng.standard_normal((T, n)) * done * (rng.random((T, n)) < 0.5)).astype(f)
    return dict(obs0=rng.standard_normal((n, D)).astype(f), next_obs=rng.standard_normal((T, n, D)).astype(f),
                actions=rng.standard_normal((T, n, A)).astype(f), log_prob=rng.standard_normal((T, n)).astype(f),
                value=(3.0 * rng.standard_normal((T, n))).astype(f), reward=rng.standard_normal((T, n)).astype(f), done=done,
                trunc=trunc, ep_reward=(10.0 * rng.standard_normal((T, n))).astype(f))


@functools.lru_cache(maxsize=None)
def _device_steps(K, n, D, A):
    return {k: _t(v) for k, v in _steps(K, n, D, A).items()}


def _fill(buf, d, steps, begin=True, trunc=False, ep=False, stream=None):
    if begin:
        buf.begin(d["obs0"], stream=stream)
    for t in range(steps):
        buf.add(d["next_obs"][t], d["actions"][t], d["log_prob"][t], d["value"][t], d["reward"][t], d["done"][t],
                trunc_value=d["trunc"][t] if trunc else None, episode_reward=d["ep_reward"][t] if ep else None, stream=stream)


def _bits(buf):
    torch.cuda.synchronize()
    return {name: getattr(buf, name).cpu().numpy().copy() for name in STORED}


def _stats(buf, clear=True):
    e = buf.episode_stats(clear=clear)
    return e["episodes"], e["length_sum"], e["return_sum"]


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


# ---- 1. the record ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n,D,A", R.SHAPES, ids=IDS)
def test_stored_rows_equal_the_inputs_bit_for_bit(K, n, D, A):
    h, d = _steps(K, n, D, A), _device_steps(K, n, D, A)
    buf = DeviceRolloutBuffer(n, K, D, A)
    _fill(buf, d, K)
    got = _bits(buf)
    assert buf.info() == {"pos": K, "overflow": 0, "bad_index": 0}
    assert np.array_equal(got["observations"][0], h["obs0"]) and np.array_equal(got["observations"][1:], h["next_obs"][:K])
    for name, key in (("actions", "actions"), ("log_probs", "log_prob"), ("values", "value"), ("rewards", "reward"), ("dones", "done")):
        assert np.array_equal(got[name].view(np.uint8), h[key][:K].view(np.uint8)), name
    assert torch.equal(buf.last_obs, d["next_obs"][K - 1])

    # the same from packed rows: strided observations, reward and a float32 done column at stride D + 2
    twin = DeviceRolloutBuffer(n, K, D, A)
    wide = torch.zeros((n, D + 5), device=DEV)
    wide[:, 2:D + 2] = d["obs0"]
    twin.begin(wide[:, 2:D + 2])
    for t in range(K):
        rows = torch.cat([d["next_obs"][t], d["reward"][t][:, None], d["done"][t][:, None].float()], dim=1).contiguous()
        twin.add_packed(rows, d["actions"][t], d["log_prob"][t], d["value"][t])
    assert _same(_bits(twin), got)
    buf.close(), twin.close()


@pytest.mark.parametrize("K,n,D,A", R.SHAPES, ids=IDS)
def test_truncation_bootstrap_is_within_one_ulp(K, n, D, A):
    h, d = _steps(K, n, D, A), _device_steps(K, n, D, A)
    gamma = 0.99
    buf = DeviceRolloutBuffer(n, K, D, A, gamma=gamma)
    _fill(buf, d, K, trunc=True)
    got = _bits(buf)["rewards"]
    exact = h["reward"][:K].astype(np.float64) + np.float64(np.float32(gamma)) * h["trunc"][:K].astype(np.float64)
    want = exact.astype(np.float32)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))
    assert np.array_equal(got[h["trunc"][:K] == 0], h["reward"][:K][h["trunc"][:K] == 0])
    buf.close()


@pytest.mark.parametrize("K,n,D,A", R.SHAPES, ids=IDS)
def test_partial_fill_overflow_and_carry_over(K, n, D, A):
    h, d = _steps(K, n, D, A), _device_steps(K, n, D, A)
    buf = DeviceRolloutBuffer(n, K, D, A)
    F = K // 2
    for name in STORED:
        t = getattr(buf, name)
        t.fill_(77 if t.dtype == torch.uint8 else -7.5)
    _fill(buf, d, F)
    buf.compute_returns_and_advantage(d["value"][K])
    got = _bits(buf)
    assert buf.info()["pos"] == F
    assert np.all(got["observations"][F + 1:] == -7.5) and np.array_equal(got["observations"][F], h["next_obs"][F - 1] if F else h["obs0"])
    for name in STORED[1:]:
        assert np.all(got[name][F:] == (77 if name == "dones" else -7.5)), name
    ref = R.RolloutBuffer(n, K, D, A)
    ref.begin(h["obs0"])
    for t in range(F):
        ref.add(h["next_obs"][t], h["actions"][t], h["log_prob"][t], h["value"][t], h["reward"][t], h["done"][t])
    ref.compute(h["value"][K].astype(np.float64))
    if F:
        bound = R.gae_bound(h["reward"][:F], h["value"][:F], ref.advantages[:F], 0.99, 0.95)
        assert np.abs(got["advantages"][:F] - ref.advantages[:F]).max() <= bound
        assert np.abs(got["returns"][:F] - ref.returns[:F]).max() <= bound

    # K + 2 steps from the start: the last two store nothing
    _fill(buf, d, K + 2)
    full = _bits(buf)
    assert buf.info() == {"pos": K, "overflow": 2, "bad_index": 0}
    assert np.array_equal(full["observations"][K], h["next_obs"][K - 1]) and np.array_equal(full["values"], h["value"][:K])
    assert torch.equal(buf.last_obs, d["next_obs"][K - 1])

    # begin() without an argument carries slot F of a partly filled buffer to slot 0
    _fill(buf, d, F)
    buf.begin()
    torch.cuda.synchronize()
    assert buf.info()["pos"] == 0
    assert np.array_equal(buf.observations[0].cpu().numpy(), h["next_obs"][F - 1] if F else h["obs0"])
    _fill(buf, d, K, begin=False)
    buf.begin()
    assert buf.info()["pos"] == 0 and np.array_equal(buf.observations[0].cpu().numpy(), h["next_obs"][K - 1])
    buf.close()


# ---- 2. GAE ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n,D,A", R.SHAPES, ids=IDS)
def test_gae_against_the_float64_checker(K, n, D, A):
    d = _device_steps(K, n, D, A)
    worst = 0.0
    for gamma, lam in R.GAE_PARAMS:
        buf = DeviceRolloutBuffer(n, K, D, A, gamma=gamma, gae_lambda=lam)
        _fill(buf, d, K)                                    # moves the cursor to K; the caller owns the storage and rewrites it below
        for case in R.GAE_CASES:
            r, v, dn, lv = R.gae_inputs(case, K, n)
            buf.rewards.copy_(_t(r)), buf.values.copy_(_t(v)), buf.dones.copy_(_t(dn))
            buf.compute_returns_and_advantage(_t(lv))
            torch.cuda.synchronize()
            a, ret = buf.advantages.cpu().numpy(), buf.returns.cpu().numpy()
            a64, r64 = R.gae(r.astype(np.float64), v.astype(np.float64), dn, lv.astype(np.float64), gamma, lam)
            bound = R.gae_bound(r, v, a64, gamma, lam)
            ratio = max(np.abs(a - a64).max(), np.abs(ret - r64).max()) / bound
            _record(f"gae {K}x{n} gamma {gamma} lambda {lam} {case}: largest error / bound = {ratio:.4f}")
            worst = max(worst, ratio)
            assert np.abs(a - a64).max() <= bound and np.abs(ret - r64).max() <= bound, (gamma, lam, case)
            if case == "all_done":                          # nothing flows: A = r - v in one rounding
                assert np.array_equal(a, r - v)
        buf.close()
    _record(f"gae {K}x{n}: largest ratio {worst:.4f}")


# ---- 3. gather ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n,D,A", R.SHAPES, ids=IDS)
def test_gather_returns_the_stored_bits(K, n, D, A):
    d = _device_steps(K, n, D, A)
    buf = DeviceRolloutBuffer(n, K, D, A)
    _fill(buf, d, K, trunc=True)
    buf.compute_returns_and_advantage(d["value"][K])
    total = K * n
    flat = RolloutBufferSamples(buf.observations[:K].reshape(total, D), buf.actions.reshape(total, A), buf.values.reshape(total),
                                buf.log_probs.reshape(total), buf.advantages.reshape(total), buf.returns.reshape(total))
    perm = torch.randperm(total, device=DEV, generator=torch.Generator(DEV).manual_seed(K * n))
    big = RolloutBufferSamples(*[torch.empty_like(f) for f in flat])
    for B in (1, 63, 64, 200):
        for t in big:
            t.fill_(-7.5)
        for start in range(0, total, B):                    # each batch into its rows of one large output: compared once per B
            buf.sample(perm[start:start + B], out=RolloutBufferSamples(*[t[start:start + B] for t in big]))
        for g, f in zip(big, flat):
            assert torch.equal(g, f[perm]), B
    idx = torch.cat([perm[:5], perm[:5], perm[:1]])         # duplicates
    for g, f in zip(buf.sample(idx), flat):
        assert torch.equal(g, f[idx])
    assert buf.info()["bad_index"] == 0

    # -1 and F * n: zero rows there, the other rows intact
    base = perm[torch.arange(6, device=DEV) % total]
    idx = torch.cat([base[:3], torch.tensor([-1], device=DEV), base[3:], torch.tensor([total], device=DEV)])
    ok = torch.tensor([1, 1, 1, 0, 1, 1, 1, 0], device=DEV, dtype=torch.bool)
    got = buf.sample(idx)
    for g, f in zip(got, flat):
        assert torch.equal(g[ok], f[idx[ok]]) and float(g[~ok].abs().max()) == 0.0
    assert buf.info()["bad_index"] == 2

    # NULL outputs are skipped
    out = RolloutBufferSamples(None, torch.full((8, A), 5.0, device=DEV), None, None, torch.full((8,), 5.0, device=DEV), None)
    buf.sample(idx.clamp(0, total - 1), out=out)
    assert torch.equal(out.actions, flat.actions[idx.clamp(0, total - 1)]) and torch.equal(out.advantages, flat.advantages[idx.clamp(0, total - 1)])

    # get(): every sample once, the final short batch included
    seen = []
    for batch in buf.get(min(64, total)):
        seen.append(batch.returns.clone())
    assert sum(len(s) for s in seen) == total and len(seen) == -(-total // min(64, total))
    assert torch.equal(torch.cat(seen).sort().values, flat.returns.sort().values)
    buf.close()


# ---- 4. episode statistics ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n,D,A", R.SHAPES[1:5], ids=IDS[1:5])
def test_episode_statistics_equal_the_checker(K, n, D, A):
    h, d = _steps(K, n, D, A), _device_steps(K, n, D, A)
    for ep in (False, True):
        buf, ref = DeviceRolloutBuffer(n, K, D, A), R.RolloutBuffer(n, K, D, A)
        half = K // 2 + 1
        for lo, hi in ((0, half), (half, K)):
            for t in range(lo, hi):
                e = h["ep_reward"][t] if ep else None
                buf.add(d["next_obs"][t], d["actions"][t], d["log_prob"][t], d["value"][t], d["reward"][t], d["done"][t],
                        episode_reward=d["ep_reward"][t] if ep else None)
                ref.add(h["next_obs"][t], h["actions"][t], h["log_prob"][t], h["value"][t], h["reward"][t], h["done"][t], episode_reward=e)
            peek = _stats(buf, clear=False)
            got, want = buf.episode_stats(clear=True), ref.episode_stats(clear=True)   # running episodes go on across the clear
            assert peek == (got["episodes"], got["length_sum"], got["return_sum"])
            assert got["episodes"] == want[2] and got["length_sum"] == want[1]
            scale = np.abs(h["ep_reward" if ep else "reward"][:K]).sum()
            assert abs(got["return_sum"] - want[0]) <= 1e-12 * scale
            if want[2]:
                assert got["ep_len_mean"] == want[1] / want[2] and abs(got["ep_rew_mean"] - want[0] / want[2]) <= 1e-12 * scale
        assert buf.episode_stats()["episodes"] == 0
        buf.close()


# ---- 5. determinism and graphs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n,D,A", R.SHAPES, ids=IDS)
def test_two_runs_and_both_graph_forms_leave_the_same_bits(K, n, D, A):
    d = _device_steps(K, n, D, A)
    idx = torch.randperm(K * n, device=DEV, generator=torch.Generator(DEV).manual_seed(1))[:min(K * n, 100)].contiguous()

    def run(buf, stream=None):
        _fill(buf, d, K, trunc=True, ep=True, stream=stream)
        buf.compute_returns_and_advantage(d["value"][K], stream=stream)

    def result(buf):
        got = buf.sample(idx)
        torch.cuda.synchronize()
        return _bits(buf), [g.cpu().numpy().copy() for g in got], _stats(buf)

    def same(x, y):
        return _same(x[0], y[0]) and all(np.array_equal(a, b) for a, b in zip(x[1], y[1])) and x[2] == y[2]

    first = DeviceRolloutBuffer(n, K, D, A)
    run(first)
    want = result(first)
    side = torch.cuda.Stream(DEV)
    second = DeviceRolloutBuffer(n, K, D, A)
    torch.cuda.synchronize()
    run(second, side)
    assert same(result(second), want)
    first.close(), second.close()

    # ONE add captured once and replayed K times fills K distinct slots: the inputs change in static buffers, the cursor on the device
    buf = DeviceRolloutBuffer(n, K, D, A)
    s = {k: torch.zeros_like(d[k][0]) for k in ("next_obs", "actions", "log_prob", "value", "reward", "done", "trunc", "ep_reward")}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        buf.add(s["next_obs"], s["actions"], s["log_prob"], s["value"], s["reward"], s["done"], trunc_value=s["trunc"],
                episode_reward=s["ep_reward"])
    buf.episode_stats(clear=True)
    with torch.cuda.stream(side):
        buf.begin(d["obs0"])
        for t in range(K):
            for k in s:
                s[k].copy_(d[k][t])
            graph.replay()
        buf.compute_returns_and_advantage(d["value"][K])
    side.synchronize()
    assert buf.info() == {"pos": K, "overflow": 0, "bad_index": 0}
    assert sum(len(b.returns) for b in buf.get(64)) == K * n            # get() goes by the device's cursor, not by the calls it saw
    assert same(result(buf), want)
    buf.close()

    # begin + K adds + compute as one graph (a single-stream chain), replayed twice: the same bits both times
    buf = DeviceRolloutBuffer(n, K, D, A)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run(buf)
    buf.episode_stats(clear=True)
    for rep in range(2):
        for name in STORED:
            getattr(buf, name).zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            graph.replay()
        side.synchronize()
        got = result(buf)
        assert _same(got[0], want[0]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1])), rep
        if rep == 0:                                        # (the second replay continues the episodes the first left running)
            assert got[2] == want[2]
    buf.close()


# ---- 6. the whole loop ------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_records_what_torch_slicing_records():
    from quadruped_gym_amd import _abi
    from quadruped_gym_amd.normalize import RunningNormalizer
    from quadruped_gym_amd.policy import FusedMlpPolicy
    from quadruped_gym_amd.sim import BatchedSim
    n, K, D, A = 70, 6, 33, 12
    task = _abi.default_task()
    task.auto_reset, task.use_fall, task.fall_height = 1, 1, 0.05
    sim = BatchedSim(n, task=task)
    sim.reset(seed=3)
    nz = RunningNormalizer(n, D)
    pol = FusedMlpPolicy(D, (64, 64), A, out_tanh=False, value=True)
    rng = np.random.default_rng(5)
    pol.set_params((0.1 * rng.standard_normal(pol.n_params)).astype(np.float32))
    buf = DeviceRolloutBuffer(n, K, D, A)
    rows = torch.zeros((n, D + 2), device=DEV)
    acts, logp, val = torch.zeros((n, A), device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    eps = torch.randn((K, n, A), device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    sim.step_device_packed(acts, rows)
    nz.step_packed(rows)
    buf.begin(rows[:, :D])
    rec = {k: [] for k in ("obs", "actions", "log_probs", "values", "rewards", "dones")}
    for t in range(K):
        rec["obs"].append(rows[:, :D].clone())
        pol.forward(rows[:, :D], acts, eps=eps[t], log_prob=logp, value=val)
        sim.step_device_packed(acts, rows)
        nz.step_packed(rows)
        buf.add_packed(rows, acts, logp, val)
        for k, src in (("actions", acts), ("log_probs", logp), ("values", val), ("rewards", rows[:, D]), ("dones", (rows[:, D + 1] != 0).to(torch.uint8))):
            rec[k].append(src.clone())
    rec["obs"].append(rows[:, :D].clone())
    pol.forward(buf.last_obs, acts, value=val)
    buf.compute_returns_and_advantage(val)
    torch.cuda.synchronize()
    assert buf.info() == {"pos": K, "overflow": 0, "bad_index": 0}
    assert torch.equal(buf.observations, torch.stack(rec["obs"]))
    for k in ("actions", "log_probs", "values", "rewards", "dones"):
        assert torch.equal(getattr(buf, k), torch.stack(rec[k])), k
    assert torch.isfinite(buf.observations).all() and float(buf.actions.abs().max()) > 0
    r, v, dn = buf.rewards.cpu().numpy(), buf.values.cpu().numpy(), buf.dones.cpu().numpy()
    a64, r64 = R.gae(r.astype(np.float64), v.astype(np.float64), dn, val.cpu().numpy().astype(np.float64), 0.99, 0.95)
    bound = R.gae_bound(r, v, a64, 0.99, 0.95)
    assert np.abs(buf.advantages.cpu().numpy() - a64).max() <= bound and np.abs(buf.returns.cpu().numpy() - r64).max() <= bound
    for h in (buf, pol, nz, sim):
        h.close()
