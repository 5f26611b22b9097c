"""The PPO loss and gradient pass on the GPU (qg_policy_ppo_grad_device, csrc/qg_policy_grad.hip) against the float64 checker of
tests/ppo_reference.py.

Tolerance of case 1: no fixed figure (the rule of tests/test_policy_gpu.py).  Per parameter tensor err = max|g - g_ref| / max|g_ref|; the
same quantity is computed for torch float32 autograd ON THE GPU on the same inputs -- the path the pass replaces -- and the pass may have
at most max(4 x torch's, 1e-6).  The same with absolute errors for every statistic but clip_fraction, which must be equal.  A tensor whose
reference gradient is all zeros (a single clipped row) must come back as exact zeros.
With QG_PPO_PARITY_OUT=<file> every case appends both paths' maxima to that file (profiles/r15/ppo_parity.txt)."""
import collections
import math
import os

import numpy as np
import pytest
import torch

import policy_reference as R
import ppo_reference as G
import ppo_torch as T
from policy_checks import DEV

from quadruped_gym_amd import _abi
from quadruped_gym_amd.policy import FusedMlpPolicy

pytestmark = pytest.mark.gpu
Samples = collections.namedtuple("Samples", G.Batch._fields)


def _record(line):
    print(line)
    out = os.environ.get("QG_PPO_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def _policy(net, actor, log_std, critic, out_tanh, reserve):
    pol = FusedMlpPolicy(net[0], net[1], net[2], out_tanh=out_tanh, value=critic is not None)
    pol.load_layers(actor, log_std, critic)
    if reserve:
        pol.reserve_grad(reserve)
    return pol


def _device_batch(batch, pad=0):
    """The batch as device tensors; ``pad`` > 0: the observations are the first columns of a wider buffer whose others hold a sentinel."""
    def t(a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    obs = t(batch.observations)
    if pad:
        wide = torch.full((obs.shape[0], obs.shape[1] + pad), 1.0e30, device=DEV)
        wide[:, :obs.shape[1]] = obs
        obs = wide[:, :batch.observations.shape[1]]
    return Samples(obs, t(batch.actions), t(batch.old_values), t(batch.old_log_prob), t(batch.advantages), t(batch.returns))


def _run(pol, dbatch, **kw):
    grad = torch.full((pol.n_params,), float("nan"), device=DEV)
    stats = torch.full((8,), float("nan"), device=DEV)
    pol.ppo_grad(dbatch, grad, stats, **kw)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), stats.cpu().numpy()


def test_batch_sizes_come_from_the_kernels_partition():
    assert (G.TILE_ROWS, G.SLOT_ROWS) == (FusedMlpPolicy.GRAD_TILE_ROWS, FusedMlpPolicy.GRAD_SLOT_ROWS)
    assert max(c.B for c in G.gradient_cases()) <= 8192


# ---- 1. gradient and statistics against the float64 reference -------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.gradient_cases(), ids=G.case_id)
def test_gradient_and_statistics_match_float64_reference(case):
    actor, log_std, critic, batch = G.build_case(case)
    kw = dict(clip_range=0.2, clip_range_vf=case.clip_range_vf, ent_coef=0.01, vf_coef=0.5)
    ref_stats, ref_grad = G.loss_and_grad(actor, log_std, critic, batch, case.out_tanh, **kw)
    t_stats, t_grads = T.gradients(actor, log_std, critic, batch, case.out_tanh, 0.2, case.clip_range_vf, 0.01, 0.5, torch.float32, DEV)
    layout = FusedMlpPolicy.param_layout(*case.net, value=case.value)
    pol = _policy(case.net, actor, log_std, critic, case.out_tanh, case.B)
    assert list(pol.param_slices().items()) == list(layout.items())
    outs = []
    for name_l, pad in (("contiguous", 0), ("strided", 3)):
        grad, stats = _run(pol, _device_batch(batch, pad), **kw)
        outs.append((grad, stats))
        assert np.isfinite(grad).all() and np.isfinite(stats).all() and stats[6] == 0 and stats[7] == 0
        lines, failures = [], []
        for (name, (off, shape)), tg in zip(layout.items(), t_grads):
            n = math.prod(shape)
            ref, got = ref_grad[off:off + n], grad[off:off + n].astype(np.float64)
            scale = np.abs(ref).max()
            if scale == 0.0:
                lines.append(f"{name}: reference all zeros")
                if np.any(got != 0.0):
                    failures.append((name, "not exact zeros"))
                continue
            err, terr = np.abs(got - ref).max() / scale, np.abs(tg.ravel() - ref).max() / scale
            bound = max(4.0 * terr, 1e-6)
            lines.append(f"{name}: fused {err:.3e} torch {terr:.3e} bound {bound:.3e}")
            if not err <= bound:
                failures.append((name, err, terr))
        for k, name in enumerate(G.STAT_NAMES):
            err, terr = abs(float(stats[k]) - ref_stats[name]), abs(t_stats[name] - ref_stats[name])
            if name == "clip_fraction":
                lines.append(f"{name}: fused {stats[k]:.6f} reference {ref_stats[name]:.6f}")
                if stats[k] != np.float32(ref_stats[name]):
                    failures.append((name, float(stats[k]), ref_stats[name]))
                continue
            bound = max(4.0 * terr, 1e-6)
            lines.append(f"{name}: fused {err:.3e} torch {terr:.3e} bound {bound:.3e}")
            if not err <= bound:
                failures.append((name, err, terr))
        _record(f"{G.case_id(case)} obs={name_l}: " + "  ".join(lines))
        assert not failures, failures
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])      # the row stride changes nothing
    pol.close()


# ---- 2. one live row, any position, same bits -----------------------------------------------------------------------------------------
def test_one_live_row_gives_the_same_bits_at_any_position():
    net, B = (33, (64, 64), 12), 100
    rng = np.random.default_rng(21)
    actor, log_std, critic = G.make_net(rng, *net)
    base = G.make_batch(rng, actor, log_std, critic, True, B)
    ratio = G.row_terms(actor, log_std, critic, base, True)[1]
    j = int(np.argmax(np.abs(ratio - 1.0) < 0.1))        # a row well inside the clip range becomes row 0, the live one
    assert abs(ratio[j] - 1.0) < 0.1
    swap = np.arange(B)
    swap[[0, j]] = [j, 0]
    base = G.Batch(*(a[swap] for a in base))
    pol = _policy(net, actor, log_std, critic, True, B)
    grads = []
    for i in (0, 15, 16, 99):
        order = np.r_[1:i + 1, 0, i + 1:B]               # row 0 of the base batch moves to position i, the others keep their order
        adv = np.zeros(B, np.float32)
        adv[i] = 0.75
        b = G.Batch(*(None if a is None else a[order] for a in base))._replace(advantages=adv)
        assert np.array_equal(b.observations[i], base.observations[0])
        grad, _ = _run(pol, _device_batch(b), ent_coef=0.0, vf_coef=0.0)
        grads.append(grad)
    lo, shape = pol.param_slices()["actor.0.weight"]
    assert np.abs(grads[0][lo:lo + math.prod(shape)]).max() > 0          # the row is not clipped: there is a gradient
    hi = pol.param_slices()["critic.0.weight"][0]
    assert not grads[0][hi:].any()                                       # vf_coef = 0: the critic's part is exact zeros
    for g in grads[1:]:
        assert np.array_equal(grads[0].view(np.uint32), g.view(np.uint32))
    pol.close()


# ---- 3. everything is written; nothing else is ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [True, False])
def test_everything_is_written_and_nothing_else(value):
    net, B = (33, (64, 64), 12), 300
    rng = np.random.default_rng(22)
    actor, log_std, critic = G.make_net(rng, *net, value=value)
    batch = G.make_batch(rng, actor, log_std, critic, False, B)
    pol = _policy(net, actor, log_std, critic, False, B)
    db = _device_batch(batch)
    assert (db.old_values is None) == (not value) and (db.returns is None) == (not value)
    acts, lp = torch.empty((B, 12), device=DEV), torch.empty(B, device=DEV)
    val = torch.empty(B, device=DEV) if value else None
    eps = torch.from_numpy(rng.standard_normal((B, 12)).astype(np.float32)).to(DEV)

    def forward():
        pol.forward(db.observations, acts, eps=eps, log_prob=lp, value=val)
        torch.cuda.synchronize()
        return [t.clone() for t in (acts, lp, val) if t is not None]
    before, params = forward(), pol.params()
    grad, stats = _run(pol, db, ent_coef=0.01)           # NaN-filled going in
    assert np.isfinite(grad).all() and np.isfinite(stats).all()
    if not value:
        assert stats[2] == 0.0                           # (the numbers of a policy without a critic are checked in case 1)
    assert np.array_equal(pol.params(), params)
    assert all(torch.equal(a, b) for a, b in zip(before, forward()))
    pol.close()


# ---- 4. reproducible -------------------------------------------------------------------------------------------------------------------
def test_reproducible_eagerly_under_graph_replay_and_after_a_larger_batch():
    net = (48, (80, 256, 48), 12)
    rng = np.random.default_rng(23)
    actor, log_std, critic = G.make_net(rng, *net)
    big = _device_batch(G.make_batch(rng, actor, log_std, critic, False, 4096, 0.2, 0.3))
    small = _device_batch(G.make_batch(rng, actor, log_std, critic, False, 17, 0.2, 0.3))
    kw = dict(clip_range_vf=0.3, ent_coef=0.01)
    fresh = _policy(net, actor, log_std, critic, False, 17)
    want_small = _run(fresh, small, **kw)
    fresh.close()

    pol = _policy(net, actor, log_std, critic, False, 4096)
    first, second = _run(pol, big, **kw), _run(pol, big, **kw)
    assert np.array_equal(first[0].view(np.uint32), second[0].view(np.uint32)) and np.array_equal(first[1].view(np.uint32), second[1].view(np.uint32))
    after = _run(pol, small, **kw)                       # scratch of the 4096-row call is still there: none of it may be read
    assert np.array_equal(after[0].view(np.uint32), want_small[0].view(np.uint32)) and np.array_equal(after[1], want_small[1])

    grad, stats = torch.zeros(pol.n_params, device=DEV), torch.zeros(8, device=DEV)
    # captured on one stream, replayed on three others: a replay carries nothing of the stream it was captured on.  (Four new streams,
    # one per hardware queue of the process: the queue assignment of streams that later tests create stays what it was)
    side, others = torch.cuda.Stream(DEV), [torch.cuda.Stream(DEV) for _ in range(3)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pol.ppo_grad(big, grad, stats, **kw)
    for other in others:
        grad.fill_(float("nan"))
        stats.fill_(float("nan"))
        torch.cuda.synchronize()
        with torch.cuda.stream(other):
            graph.replay()
        other.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(grad.cpu().numpy().view(np.uint32), first[0].view(np.uint32))
        assert np.array_equal(stats.cpu().numpy().view(np.uint32), first[1].view(np.uint32))
    del graph
    pol.close()


# ---- 5. refusals, and the repack after an update ---------------------------------------------------------------------------------------
def test_refusals():
    net, B = (33, (64, 64), 12), 64
    rng = np.random.default_rng(24)
    actor, log_std, critic = G.make_net(rng, *net)
    batch = G.make_batch(rng, actor, log_std, critic, False, B)
    db = _device_batch(batch)
    pol = _policy(net, actor, log_std, critic, False, 0)
    grad, stats = torch.zeros(pol.n_params, device=DEV), torch.zeros(8, device=DEV)
    with pytest.raises(_abi.QuadGymError):
        pol.ppo_grad(db, grad, stats)                    # nothing reserved
    with pytest.raises(_abi.QuadGymError):
        pol.reserve_grad(0)
    pol.reserve_grad(B - 1)
    with pytest.raises(_abi.QuadGymError):
        pol.ppo_grad(db, grad, stats)                    # B > max_batch
    pol.reserve_grad(B)                                  # growing is allowed
    pol.ppo_grad(db, grad, stats)
    for bad in (dict(clip_range=0.0), dict(clip_range=-0.2), dict(clip_range=float("nan")), dict(ent_coef=float("inf"))):
        with pytest.raises((_abi.QuadGymError, ValueError)):
            pol.ppo_grad(db, grad, stats, **bad)
    with pytest.raises(ValueError):
        pol.ppo_grad(db, grad.double(), stats)
    with pytest.raises(ValueError):
        pol.ppo_grad(db, grad[:-1], stats)
    with pytest.raises(ValueError):
        pol.ppo_grad(db, grad.cpu(), stats)
    with pytest.raises(ValueError):
        pol.ppo_grad(db._replace(actions=db.actions[:, :-1].contiguous()), grad, stats)
    with pytest.raises(ValueError):
        pol.ppo_grad(db._replace(advantages=db.advantages[:-1]), grad, stats)
    with pytest.raises(ValueError):
        pol.ppo_grad(db._replace(returns=None), grad, stats)
    with pytest.raises(ValueError):
        pol.ppo_grad(db._replace(old_values=None), grad, stats, clip_range_vf=0.3)
    pol.ppo_grad(db._replace(old_values=None), grad, stats)              # no value clipping: old_values is not read
    torch.cuda.synchronize()
    assert torch.isfinite(grad).all()
    pol.close()


def test_a_call_after_update_from_uses_the_new_parameters():
    net, B = (20, (16, 32, 240), 4), 200
    rng = np.random.default_rng(25)
    actor, log_std, critic = G.make_net(rng, *net)
    pol = _policy(net, actor, log_std, critic, False, B)
    actor2, log_std2, critic2 = G.make_net(rng, *net)
    batch = G.make_batch(rng, actor2, log_std2, critic2, False, B, 0.2, 0.3)
    db = _device_batch(batch)
    kw = dict(clip_range=0.2, clip_range_vf=0.3, ent_coef=0.01, vf_coef=0.5)
    _run(pol, db, **kw)                                  # with the old parameters
    pol.update_from(torch.from_numpy(R.flatten(actor2, log_std2, critic2)).to(DEV))
    grad, stats = _run(pol, db, **kw)
    ref_stats, ref_grad = G.loss_and_grad(actor2, log_std2, critic2, batch, False, **kw)
    _, t_grads = T.gradients(actor2, log_std2, critic2, batch, False, 0.2, 0.3, 0.01, 0.5, torch.float32, DEV)
    for (name, (off, shape)), tg in zip(pol.param_slices().items(), t_grads):
        n = math.prod(shape)
        scale = np.abs(ref_grad[off:off + n]).max()
        err, terr = np.abs(grad[off:off + n] - ref_grad[off:off + n]).max() / scale, np.abs(tg.ravel() - ref_grad[off:off + n]).max() / scale
        assert err <= max(4.0 * terr, 1e-6), (name, err, terr)
    assert stats[5] == np.float32(ref_stats["clip_fraction"])
    pol.close()


# ---- 6. first-epoch identity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_tanh", [False, True])
def test_first_epoch_has_no_clipped_row(out_tanh):
    net, B = (260, (32, 48), 7), 1000
    rng = np.random.default_rng(26)
    actor, log_std, critic = G.make_net(rng, *net)
    pol = _policy(net, actor, log_std, critic, out_tanh, B)
    obs = torch.from_numpy((rng.standard_normal((B, net[0])) * np.logspace(-2, 1, net[0])).astype(np.float32)).to(DEV)
    eps = torch.from_numpy(rng.standard_normal((B, net[2])).astype(np.float32)).to(DEV)
    acts, lp, val = torch.empty((B, net[2]), device=DEV), torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    pol.forward(obs, acts, eps=eps, log_prob=lp, value=val)
    adv = torch.from_numpy(rng.standard_normal(B).astype(np.float32)).to(DEV)
    ret = torch.from_numpy(rng.standard_normal(B).astype(np.float32)).to(DEV)
    grad, stats = _run(pol, Samples(obs, acts, val, lp, adv, ret), clip_range_vf=0.3)
    # clip_fraction; approx_kl = mean(lr^2 / 2 ..) where lr is the float32 rounding of a log-probability: |lr| < 1e-3 by a wide margin
    assert stats[5] == 0.0 and abs(stats[4]) <= 1e-6
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0
    pol.close()


# ---- 7. it trains ----------------------------------------------------------------------------------------------------------------------
TRAIN_STEPS, TRAIN_RATE = 200, 1e-3      # the float64 loop below ends at 0.004 x its initial value_loss with these: no adjustment needed


def test_it_trains():
    net, B = (33, (64, 64), 12), 512
    rng = np.random.default_rng(7)
    actor, log_std, critic = G.make_net(rng, *net)
    batch = G.make_batch(rng, actor, log_std, critic, False, B)._replace(advantages=np.zeros(B, np.float32))
    layout = FusedMlpPolicy.param_layout(*net, value=True)

    def unflatten(flat):
        def tw(name):
            return [tuple(flat[off:off + math.prod(shape)].reshape(shape) for off, shape in (layout[f"{name}.{k}.weight"], layout[f"{name}.{k}.bias"]))
                    for k in range(len(net[1]) + 1)]
        off, shape = layout["log_std"]
        return tw("actor"), flat[off:off + shape[0]], tw("critic")

    # the float64 loop: the checker's gradient and Adam (beta 0.9 / 0.999, eps 1e-8: torch's defaults) in NumPy
    flat = R.flatten(actor, log_std, critic).astype(np.float64)
    m, v, first = np.zeros_like(flat), np.zeros_like(flat), None
    for t in range(1, TRAIN_STEPS + 1):
        a, ls, c = unflatten(flat)
        stats, g = G.loss_and_grad(a, ls, c, batch, False, 0.2, None, 0.0, 1.0)
        first = stats["value_loss"] if first is None else first
        m, v = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
        flat = flat - TRAIN_RATE * (m / (1 - 0.9 ** t)) / (np.sqrt(v / (1 - 0.999 ** t)) + 1e-8)
    a, ls, c = unflatten(flat)
    last = G.loss_and_grad(a, ls, c, batch, False, 0.2, None, 0.0, 1.0)[0]["value_loss"]
    assert last < 0.25 * first, (first, last)

    pol = _policy(net, actor, log_std, critic, False, B)
    db = _device_batch(batch)
    flat_t = torch.from_numpy(R.flatten(actor, log_std, critic)).to(DEV).requires_grad_(True)
    grad, stats_t = torch.zeros_like(flat_t), torch.zeros(8, device=DEV)
    flat_t.grad = grad
    opt = torch.optim.Adam([flat_t], TRAIN_RATE)
    losses = []
    for t in range(TRAIN_STEPS + 1):
        pol.ppo_grad(db, grad, stats_t, ent_coef=0.0, vf_coef=1.0)
        if t in (0, TRAIN_STEPS):
            losses.append(float(stats_t[2]))
        if t < TRAIN_STEPS:
            opt.step()
            pol.update_from(flat_t)
    print(f"value_loss: float64 loop {first:.4f} -> {last:.5f}; device loop {losses[0]:.4f} -> {losses[1]:.5f}")
    assert abs(losses[0] - first) <= 1e-5 * first and losses[1] < 0.5 * losses[0], losses
    pol.close()
