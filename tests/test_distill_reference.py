"""The float64 checker of the distillation pass (tests/distill_reference.py) against torch: its gradient equals float64 autograd of the
torch statement of the loss on every case of the GPU module, the KL term equals torch.distributions.kl_divergence of two Normals, the
entries the header calls exact zeros are zeros, and 20 steps of the checker's gradient through adam_reference's Adam lower sq_err on
the fixed batch the GPU module replays."""
import math

import numpy as np
import pytest
import torch

import adam_reference as A
import distill_reference as D
import policy_reference as R
import ppo_reference as G

from quadruped_gym_amd.policy import FusedMlpPolicy


def test_the_case_list_covers_the_partition_and_the_options():
    cases = D.gradient_cases()
    assert len({D.case_id(c) for c in cases}) == len(cases) and max(c.B for c in cases) <= 8192
    assert FusedMlpPolicy.DISTILL_STAT_NAMES == D.STAT_NAMES
    for net in G.NETS:
        assert {c.B for c in cases if c.net == net} >= set(G.BATCHES)
        for field, values in (("out_tanh", (False, True)), ("mode", D.MODES), ("weights", D.WEIGHTS), ("value", (False, True))):
            assert {getattr(c, field) for c in cases if c.net == net} == set(values), (net, field)
    for B in G.BATCHES:
        for field, values in (("out_tanh", (False, True)), ("mode", D.MODES), ("weights", D.WEIGHTS), ("value", (False, True))):
            assert {getattr(c, field) for c in cases if c.B == B} == set(values), (B, field)
    assert {c.mode for c in cases if c.net == G.WIDE} == set(D.MODES) and {c.B for c in cases if c.net == G.WIDE} == {100}
    assert {c.net[2] for c in cases} >= {1, 4, 7, 12}


@pytest.mark.parametrize("case", D.gradient_cases(), ids=D.case_id)
def test_reference_gradient_equals_float64_autograd(case):
    data = D.build_case(case)
    kw = D.kwargs(case, data)
    stats, grad = D.loss_and_grad(data.actor, data.log_std, data.critic, data.obs, data.target, **kw)
    t_stats, t_grads = D.torch_gradients(data, **kw)
    layout = FusedMlpPolicy.param_layout(*case.net, value=case.value)
    assert len(layout) == len(t_grads) and grad.shape == (R.param_count(*case.net, case.value),)
    for (name, (off, shape)), tg in zip(layout.items(), t_grads):
        ref = grad[off:off + math.prod(shape)]
        scale = max(np.abs(tg).max(), 1e-300)
        assert np.abs(ref - tg.ravel()).max() <= 1e-10 * scale, (name, np.abs(ref - tg.ravel()).max() / scale)
    for name in D.STAT_NAMES:
        assert abs(stats[name] - t_stats[name]) <= 1e-12 * max(1.0, abs(t_stats[name])), name
    if data.weights is not None and case.weights == "zeros" and case.B >= 100:
        assert (data.weights == 0).mean() > 0.2 and (data.weights != 0).mean() > 0.5


def test_kl_term_is_torchs_kl_divergence_of_two_normals():
    rng = np.random.default_rng(31)
    t, mu = torch.from_numpy(rng.standard_normal((50, 7))), torch.from_numpy(rng.standard_normal((50, 7)))
    lt, ls = torch.from_numpy(rng.uniform(-2, 0.5, 7)), torch.from_numpy(rng.uniform(-2, 0.5, 7))
    w = torch.from_numpy(rng.uniform(0, 2, 50))
    want = torch.distributions.kl_divergence(torch.distributions.Normal(t, lt.exp().expand(50, 7)),
                                             torch.distributions.Normal(mu, ls.exp().expand(50, 7))).sum(dim=1)
    got = D.torch_loss(mu, ls, t, "kl", 0.3, lt, w)
    assert abs(float(got) - 0.3 * float((w * want).mean())) <= 1e-13 * abs(float(got))
    # and the NumPy checker's statistic on a net whose means those are: a one-layer identity "actor"
    actor = [(np.eye(7), np.zeros(7))]
    stats, _ = D.loss_and_grad(actor, ls.numpy(), None, mu.numpy(), t.numpy(), False, "kl", 0.3, lt.numpy(), w.numpy())
    assert abs(stats["loss"] - float(got)) <= 1e-13 * abs(float(got)) and abs(stats["kl"] - float(got) / 0.3) <= 1e-12
    # equal distributions: the divergence is zero and so is the gradient on log_std
    stats, grad = D.loss_and_grad(actor, ls.numpy(), None, mu.numpy(), mu.numpy(), False, "kl", 1.0, ls.numpy(), None)
    assert abs(stats["kl"]) <= 1e-14 and np.abs(grad).max() <= 1e-14


@pytest.mark.parametrize("mode", D.MODES)
def test_the_exact_zeros_of_the_header(mode):
    rng = np.random.default_rng(32)
    net, B = (33, (64, 64), 12), 100
    data = D.make_data(rng, net, B, True, True, "zeros")
    kw = dict(out_tanh=True, mode=mode, coef=1.3, target_log_std=data.target_log_std if mode == "kl" else None)
    stats, grad = D.loss_and_grad(data.actor, data.log_std, data.critic, data.obs, data.target, weights=data.weights, **kw)
    layout = FusedMlpPolicy.param_layout(*net, value=True)
    lo = layout["critic.0.weight"][0]
    assert not grad[lo:].any() and not np.signbit(grad[lo:]).any()                     # the critic: +0.0
    off = layout["log_std"][0]
    assert (mode == "mse") == (not grad[off:off + 12].any()) and grad[:off].any()      # log_std: +0.0 in MSE mode only
    assert (stats["kl"] == 0.0) == (mode == "mse") and stats["weight_sum"] == float(data.weights.astype(np.float64).sum())
    # rows of weight zero contribute nothing: the batch without them, scaled by its size, has the same gradient and sums
    live = data.weights != 0
    assert 0 < live.sum() < B
    sub = data._replace(obs=data.obs[live], target=data.target[live], weights=data.weights[live])
    s_stats, s_grad = D.loss_and_grad(sub.actor, sub.log_std, sub.critic, sub.obs, sub.target, weights=sub.weights, **kw)
    scale = live.sum() / B
    assert np.abs(grad - scale * s_grad).max() <= 1e-13 * np.abs(grad).max()
    assert abs(stats["loss"] - scale * s_stats["loss"]) <= 1e-13 * abs(stats["loss"]) and stats["max_abs_err"] == s_stats["max_abs_err"]
    # and what they hold does not matter (the header's 1/B, not 1/sum w): other observations and targets in the dead rows
    other = data._replace(obs=np.where(live[:, None], data.obs, 3.0).astype(np.float32), target=np.where(live[:, None], data.target, -9.0).astype(np.float32))
    o_stats, o_grad = D.loss_and_grad(other.actor, other.log_std, other.critic, other.obs, other.target, weights=other.weights, **kw)
    assert np.array_equal(o_grad, grad) and o_stats == stats
    # no live row at all: every entry and every statistic is zero
    z_stats, z_grad = D.loss_and_grad(data.actor, data.log_std, data.critic, data.obs, data.target, weights=np.zeros(B, np.float32), **kw)
    assert not z_grad.any() and all(z_stats[k] == 0.0 for k in D.STAT_NAMES)


def test_twenty_steps_of_adam_lower_the_squared_error():
    """The precondition of the GPU module's replay: with these seeds and this rate the float64 loop alone shows the descent."""
    data = D.replay_data()
    flat = R.flatten(data.actor, data.log_std, data.critic).astype(np.float64)
    m, v, t, errs = np.zeros_like(flat), np.zeros_like(flat), 0, []
    for _ in range(D.REPLAY_STEPS + 1):
        actor, log_std, critic = D.unflatten(flat, D.REPLAY_NET, True)
        stats, grad = D.loss_and_grad(actor, log_std, critic, data.obs, data.target)
        errs.append(stats["sq_err"])
        flat, m, v, t, _ = A.clip_and_adam(flat, m, v, t, grad, D.REPLAY_RATE, A.BETA1, A.BETA2, A.EPS, A.MAX_NORM, np.float64)
    print("sq_err:", " ".join(f"{e:.4f}" for e in errs))
    assert errs[-1] < 0.5 * errs[0] and errs[0] > 0.1, (errs[0], errs[-1])
