"""The loop and the auditor of tests/ppo_iteration_reference.py, on the CPU: the float64 loop against an independently written torch
float64 loop, the census of the committed seeds (conditions on the inputs, not measurements), and the auditor's sensitivity -- no
finding on a clean float32 run, a finding at the right stage for every deliberate wiring error."""
import functools

import numpy as np
import pytest
import torch

import normalize_reference as NR
import ppo_iteration_reference as P
import ppo_reference as G
import ppo_torch as T
from policy_checks import bound as forward_bound         # the forward pass's tolerance rule

CASE_NAMES = list(P.CASES)


@functools.lru_cache(maxsize=None)
def _recording(name, dtype, miswire=None):
    return P.run_numpy(P.CASES[name], np.dtype(dtype).type, miswire)


def _forward_baseline(actor, log_std, critic, obs, eps, out_tanh):
    """The torch float32 modules on the CPU: (actions, log_prob, value) as tests/test_policy_gpu.py forms them."""
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(obs, np.float32))
        mean = T.tower(actor, out_tanh, torch.float32)(x)
        std = torch.from_numpy(np.array(log_std, np.float32)).exp()
        act = mean if eps is None else mean + std * torch.from_numpy(np.array(eps, np.float32))
        lp = torch.distributions.Normal(mean, std).log_prob(act).sum(-1)
        val = T.tower(critic, False, torch.float32)(x)[:, 0]
    return act.numpy(), lp.numpy(), val.numpy()


def _audit(case, rec):
    return P.audit(case, rec, functools.partial(T.gradients, dtype=torch.float32, device="cpu"), _forward_baseline, forward_bound)


# ---- 1. the float64 loop against torch --------------------------------------------------------------------------------------------------
def _torch_loop(case):
    """The listing in torch float64 on the same tables and permutations: modules, autograd on ppo_torch.loss, clip_grad_norm_ and
    torch.optim.Adam; GAE written out here.  (The normaliser is the float64 checker itself: both loops are defined on its outputs.)
    Returns the final parameter tensors in the canonical order."""
    f64 = torch.float64
    tb = P.tables(case)
    n, K, D, A = case.n, case.K, case.D, case.A
    actor, log_std, critic = P.unflatten(tb.flat0.copy(), case)
    actor_m, critic_m = T.tower(actor, case.out_tanh, f64), T.tower(critic, False, f64)
    ls = torch.nn.Parameter(torch.from_numpy(np.array(log_std)).to(f64))
    tensors = list(actor_m.parameters()) + [ls] + list(critic_m.parameters())
    opt = torch.optim.Adam(tensors, case.learning_rate)
    nz = NR.Normalizer(n, D, gamma=P.GAMMA)

    def env(raw, done, act):
        reward = -((act - 0.5 * torch.tanh(torch.from_numpy(np.array(raw[:, :A])).to(f64))) ** 2).mean(1)
        obs_n, rew_n = nz.step(raw, reward.numpy(), done)
        return torch.from_numpy(obs_n).to(f64), torch.from_numpy(rew_n).to(f64)

    def policy(obs, eps):
        with torch.no_grad():
            mean, std = actor_m(obs), ls.exp()
            act = mean + std * torch.from_numpy(eps).to(f64)
            return act, torch.distributions.Normal(mean, std).log_prob(act).sum(-1), critic_m(obs)[:, 0]

    obs, _ = env(tb.raw_pre[0], tb.done_pre[0], torch.zeros((n, A), dtype=f64))
    obs, _ = env(tb.raw_pre[1], tb.done_pre[1], policy(obs, tb.eps_warm)[0])
    for it in range(case.iterations):
        o, a, lp, v, r = (torch.zeros(s, dtype=f64) for s in ((K, n, D), (K, n, A), (K, n), (K, n), (K, n)))
        for t in range(K):
            o[t] = obs
            a[t], lp[t], v[t] = policy(obs, tb.eps[it, t])
            obs, r[t] = env(tb.raw[it, t], tb.done[it, t], a[t])
        with torch.no_grad():
            next_v = critic_m(obs)[:, 0]
        live = 1.0 - torch.from_numpy(tb.done[it].astype(np.float64))
        adv, run = torch.zeros((K, n), dtype=f64), torch.zeros(n, dtype=f64)
        for t in reversed(range(K)):                        # SB3's compute_returns_and_advantage: episode_starts[t + 1] is dones[t]
            delta = r[t] + P.GAMMA * next_v * live[t] - v[t]
            run = delta + P.GAMMA * P.GAE_LAMBDA * live[t] * run
            adv[t], next_v = run, v[t]
        ret = adv + v
        flat = [x.reshape((K * n,) + x.shape[2:]) for x in (o, a, v, lp, adv, ret)]
        for epoch in range(case.epochs):
            perm = torch.from_numpy(tb.perms[it, epoch])
            for start in range(0, K * n, case.batch_size):
                idx = perm[start:start + case.batch_size]
                batch = G.Batch(*[x[idx] for x in flat])
                batch = batch._replace(advantages=(batch.advantages - batch.advantages.mean()) / (batch.advantages.std() + 1e-8))
                opt.zero_grad()
                total, _ = T.loss(actor_m, ls, critic_m, batch, P.CLIP_RANGE, case.clip_range_vf, P.ENT_COEF, P.VF_COEF)
                total.backward()
                torch.nn.utils.clip_grad_norm_(tensors, P.MAX_GRAD_NORM)
                opt.step()
    return [p.detach().numpy() for p in tensors]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_float64_loop_equals_the_torch_float64_loop(name):
    case = P.CASES[name]
    final = _recording(name, "float64").iterations[-1]["minibatches"][-1]["flat_after"]
    assert final.dtype == np.float64
    moved = np.abs(final - P.tables(case).flat0).max()
    assert moved > 1e-4                                      # eight Adam steps of 3e-4 did move the parameters
    for (tensor, off, size), want in zip(P.tensor_slices(case), _torch_loop(case)):
        err = np.abs(final[off:off + size] - want.ravel()).max() / np.abs(want).max()
        assert err <= 1e-9, (tensor, err)


# ---- 2. census of the committed seeds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_census_of_the_committed_seed(name):
    case = P.CASES[name]
    assert (case.learning_rate, P.CLIP_RANGE) == (3e-4, 0.2)
    c = P.census(case, _recording(name, "float64"))
    print(name, c)
    assert len(c["gaps"]) == case.iterations * case.epochs * 2                   # two minibatches per epoch, the second short
    assert c["min_gap"] >= 10 * G.BAND, c["gaps"]          # every minibatch; for `wide` a value-clip boundary counts too
    assert max(c["clip_fractions"]) >= 0.04, c["clip_fractions"]
    assert min(c["episodes"]) >= 1 and c["overflow"] == 0


def test_the_cases_are_the_shapes_they_claim():
    p, w = P.CASES["plain"], P.CASES["wide"]
    assert (p.n, p.K, p.D, p.A, p.hidden, p.out_tanh, p.clip_range_vf, p.batch_size) == (131, 8, 33, 12, (64, 64), False, None, 600)
    assert (w.n, w.K, w.D, w.A, w.hidden, w.out_tanh, w.clip_range_vf, w.batch_size) == (70, 5, 260, 7, (32, 48), True, 0.3, 200)
    for c in (p, w):
        assert (c.iterations, c.epochs) == (2, 2)
    assert p.n * p.K - p.batch_size == 448 and p.batch_size == G.SLOT_ROWS + 88 and 88 % G.TILE_ROWS == 8
    assert w.n * w.K - w.batch_size == 150 and 200 % G.TILE_ROWS and 150 % G.TILE_ROWS


# ---- 3. the auditor's sensitivity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_a_clean_float32_run_has_no_finding(name):
    rec = _recording(name, "float32")
    assert all(a.dtype != np.float64 for path, a in rec.arrays() if "norm_state" not in path and "return_sum" not in path)
    lines = []
    assert P.audit(P.CASES[name], rec, functools.partial(T.gradients, dtype=torch.float32, device="cpu"), _forward_baseline, forward_bound,
                   report=lines.append) == []
    assert len(lines) == 8 + 1 and all(s in lines[-1] for s in P.STAGES if s not in ("storage", "gather", "first_minibatch", "parameters"))


@pytest.mark.parametrize("miswire", list(P.MISWIRES))
@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_miswiring_is_found_at_its_stage(name, miswire):
    findings = _audit(P.CASES[name], _recording(name, "float32", miswire))
    stages = {f.stage for f in findings}
    print(miswire, sorted(stages), findings[:3])
    assert P.MISWIRES[miswire] in stages, (miswire, stages)
    # the stages upstream of the error stay clean: the audit is teacher-forced, so nothing is blamed on the normaliser or on GAE
    assert not stages & {"normaliser", "gae"}, stages


def test_two_runs_of_the_loop_leave_the_same_bits_and_a_miswired_one_does_not():
    case = P.CASES["wide"]
    assert P.differences(_recording("wide", "float32"), P.run_numpy(case, np.float32)) == []
    assert P.differences(_recording("wide", "float32"), _recording("wide", "float32", "last_values_slot"))
