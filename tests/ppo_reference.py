"""Float64 restatement of the PPO loss and gradient pass (include/quadgym.h, "the PPO loss and its gradient"), written from the
formulae of SB3 2.x ``PPO.train`` and their derivatives by hand, not from the kernel: the checker of tests/test_ppo_reference.py
(against torch float64 autograd) and tests/test_ppo_gpu.py.  NumPy only."""
import collections
import math

import numpy as np

import policy_reference as R

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
BAND = 1e-4                      # rows this close to a clip boundary are redrawn: the gradient is discontinuous there
STAT_NAMES = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")

Batch = collections.namedtuple("Batch", ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns"])


def _tower(layers, x, out_tanh):
    """Forward pass keeping every layer's input: ``(inputs, output)``; the output has tanh applied when ``out_tanh``."""
    hs, h = [], np.asarray(x, np.float64)
    for k, (W, b) in enumerate(layers):
        hs.append(h)
        h = h @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        if k < len(layers) - 1 or out_tanh:
            h = np.tanh(h)
    return hs, h


def _back(layers, hs, delta):
    """``delta`` = d loss / d (pre-activation of the last layer), ``[B, out]``: the ``[(dW, db), ...]`` of the tower."""
    grads = [None] * len(layers)
    for k in range(len(layers) - 1, -1, -1):
        grads[k] = (delta.T @ hs[k], delta.sum(0))
        if k:
            delta = (delta @ np.asarray(layers[k][0], np.float64)) * (1.0 - hs[k] ** 2)
    return grads


def row_terms(actor, log_std, critic, batch, out_tanh, clip_range=0.2, clip_range_vf=None):
    """Per-row ``(logp, ratio, v)`` in float64 (``v`` None without a critic)."""
    _, mean = _tower(actor, batch.observations, out_tanh)
    ls = np.asarray(log_std, np.float64)
    z = (np.asarray(batch.actions, np.float64) - mean) / np.exp(ls)
    logp = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1)
    ratio = np.exp(logp - np.asarray(batch.old_log_prob, np.float64))
    v = _tower(critic, batch.observations, False)[1][:, 0] if critic else None
    return logp, ratio, v


def classes(actor, log_std, critic, batch, out_tanh, clip_range=0.2, clip_range_vf=None):
    """Fractions of rows ``(clipped high, clipped low, value-clipped)`` and the smallest distance of any row to a clip boundary."""
    _, r, v = row_terms(actor, log_std, critic, batch, out_tanh)
    adv = np.asarray(batch.advantages, np.float64)
    c = float(clip_range)
    hi, lo = np.mean((adv > 0) & (r > 1 + c)), np.mean((adv < 0) & (r < 1 - c))
    gap = min(np.abs(r - (1 + c)).min(), np.abs(r - (1 - c)).min())
    vc = 0.0
    if critic and clip_range_vf:
        d = np.abs(v - np.asarray(batch.old_values, np.float64))
        vc, gap = np.mean(d >= clip_range_vf), min(gap, np.abs(d - clip_range_vf).min())
    return hi, lo, vc, gap


def loss_and_grad(actor, log_std, critic, batch, out_tanh=False, clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5):
    """``(stats, grad)``: ``stats`` a dict over ``STAT_NAMES``, ``grad`` the float64 gradient of ``loss`` in the canonical flat order."""
    B = len(batch.observations)
    c, ls = float(clip_range), np.asarray(log_std, np.float64)
    adv = np.asarray(batch.advantages, np.float64)
    hs_a, mean = _tower(actor, batch.observations, out_tanh)
    sigma = np.exp(ls)
    z = (np.asarray(batch.actions, np.float64) - mean) / sigma
    logp = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1)
    lr = logp - np.asarray(batch.old_log_prob, np.float64)
    r = np.exp(lr)
    policy_loss = -np.mean(np.minimum(adv * r, adv * np.clip(r, 1 - c, 1 + c)))
    entropy_loss = -np.sum(0.5 + HALF_LOG_2PI + ls)
    dlogp = -(adv * r) / B
    dlogp[((adv > 0) & (r > 1 + c)) | ((adv < 0) & (r < 1 - c))] = 0.0
    dmean = dlogp[:, None] * z / sigma
    if out_tanh:
        dmean = dmean * (1.0 - mean ** 2)
    g_actor = _back(actor, hs_a, dmean)
    g_log_std = (dlogp[:, None] * (z * z - 1.0)).sum(0) - ent_coef
    value_loss, g_critic = 0.0, []
    if critic:
        hs_c, v = _tower(critic, batch.observations, False)
        v, ret = v[:, 0], np.asarray(batch.returns, np.float64)
        vp, live = v, np.ones(B, bool)
        if clip_range_vf is not None and clip_range_vf > 0:
            ov = np.asarray(batch.old_values, np.float64)
            vp = ov + np.clip(v - ov, -clip_range_vf, clip_range_vf)
            live = np.abs(v - ov) < clip_range_vf
        value_loss = np.mean((ret - vp) ** 2)
        g_critic = _back(critic, hs_c, (vf_coef * 2.0 * (vp - ret) / B * live)[:, None])
    stats = {"loss": policy_loss + ent_coef * entropy_loss + vf_coef * value_loss, "policy_loss": policy_loss, "value_loss": value_loss,
             "entropy_loss": entropy_loss, "approx_kl": np.mean((r - 1.0) - lr), "clip_fraction": np.mean(np.abs(r - 1.0) > c)}
    parts = [p.ravel() for Wb in g_actor for p in Wb] + [g_log_std] + [p.ravel() for Wb in g_critic for p in Wb]
    return stats, np.concatenate(parts)


def make_net(rng, obs_dim, hidden, act_dim, value=True, sigma=0.3):
    """``(actor, log_std, critic)``: torch.nn.Linear's default initialisation, a wider action head so that the actor's gradient is
    not tiny, ``log_std`` spread around ``log(sigma)``."""
    actor = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, act_dim), "linear")
    critic = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, 1), "linear") if value else None
    log_std = (math.log(sigma) + rng.uniform(-0.2, 0.2, act_dim)).astype(np.float32)
    return actor, log_std, critic


def make_batch(rng, actor, log_std, critic, out_tanh, B, clip_range=0.2, clip_range_vf=None, noise=0.3):
    """The input recipe: observations with per-column scales 0.01 .. 10, actions ``mean + sigma N(0, 1)``, ``old_log_prob = logp +
    N(0, noise)``, ``advantages ~ N(0, 1)``, ``old_values = v + N(0, noise)``, ``returns ~ N(0, 1)``, all float32.  A row whose float64
    ratio lies within ``BAND`` of ``1 +- clip_range``, or whose ``|v - old_values|`` within ``BAND`` of ``clip_range_vf``, gets its
    ``old_log_prob`` / ``old_values`` redrawn."""
    obs_dim, act_dim = actor[0][0].shape[1], actor[-1][0].shape[0]
    obs = (rng.standard_normal((B, obs_dim)) * np.logspace(-2, 1, obs_dim)).astype(np.float32)
    mean = R.mlp(actor, obs, out_tanh)
    actions = (mean + np.exp(np.asarray(log_std, np.float64)) * rng.standard_normal((B, act_dim))).astype(np.float32)
    adv = rng.standard_normal(B).astype(np.float32)
    ret = rng.standard_normal(B).astype(np.float32)
    probe = Batch(obs, actions, None, np.zeros(B, np.float32), adv, ret)
    logp, _, v = row_terms(actor, log_std, critic, probe, out_tanh)
    old_lp = (logp + noise * rng.standard_normal(B)).astype(np.float32)
    c = float(clip_range)
    for _ in range(100):
        r = np.exp(logp - old_lp.astype(np.float64))
        bad = (np.abs(r - (1 + c)) < BAND) | (np.abs(r - (1 - c)) < BAND)
        if not bad.any():
            break
        old_lp[bad] = (logp[bad] + noise * rng.standard_normal(int(bad.sum()))).astype(np.float32)
    old_v = None
    if critic:
        old_v = (v + noise * rng.standard_normal(B)).astype(np.float32)
        for _ in range(100):
            if not clip_range_vf:
                break
            bad = np.abs(np.abs(v - old_v.astype(np.float64)) - clip_range_vf) < BAND
            if not bad.any():
                break
            old_v[bad] = (v[bad] + noise * rng.standard_normal(int(bad.sum()))).astype(np.float32)
    return Batch(obs, actions, old_v, old_lp, adv, ret if critic else None)


# ---- the cases of tests/test_ppo_gpu.py (test_ppo_reference.py checks the class sizes of those with B >= 256) -----------------------------
TILE_ROWS, SLOT_ROWS = 16, 512       # FusedMlpPolicy.GRAD_TILE_ROWS / GRAD_SLOT_ROWS (the GPU test asserts they agree)
NETS = ((3, (16,), 1), (33, (64, 64), 12), (260, (32, 48), 7), (20, (16, 32, 240), 4), (48, (80, 256, 48), 12))
WIDE = (260, (256, 256, 128), 12)
# 1, 15, 16, 17: the edges of a tile; one slot exactly and one row past it; three slots and a fourth of 40 rows (2 tiles and a half)
BATCHES = (1, 15, 16, 17, SLOT_ROWS, SLOT_ROWS + 1, 3 * SLOT_ROWS + 40)
Case = collections.namedtuple("Case", ["net", "B", "out_tanh", "clip_range_vf", "value", "seed"])


def gradient_cases():
    """Every net at every batch size; ``out_tanh``, value clipping, the critic and (in the test) the row stride vary along the list so
    that each combination of net and option, and of batch size and option, occurs."""
    cases = []
    for i, net in enumerate(NETS):
        for j, B in enumerate(BATCHES):
            k = i + j
            cases.append(Case(net, B, bool(k % 2), 0.3 if (k // 2) % 2 else None, (i + 2 * j) % 3 != 0, 1000 + 10 * i + j))
    # the options on one net and batch, in full
    for out_tanh in (False, True):
        for cv in (None, 0.3):
            for value in (False, True):
                cases.append(Case(NETS[1], 600, out_tanh, cv, value, 2000 + len(cases)))
    cases.append(Case(WIDE, 100, False, 0.3, True, 3000))
    return cases


def case_id(case):
    return "%d-%s-%d-B%d-tanh%d-cv%s-critic%d" % (case.net[0], "-".join(map(str, case.net[1])), case.net[2], case.B, case.out_tanh,
                                                  case.clip_range_vf or 0, case.value)


def build_case(case):
    """``(actor, log_std, critic, batch)`` of a case: seeded, so the CPU census and the GPU test see the same data."""
    rng = np.random.default_rng(case.seed)
    actor, log_std, critic = make_net(rng, *case.net, value=case.value)
    batch = make_batch(rng, actor, log_std, critic, case.out_tanh, case.B, 0.2, case.clip_range_vf)
    return actor, log_std, critic, batch
