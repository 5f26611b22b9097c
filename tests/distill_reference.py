"""Float64 restatement of the distillation loss and gradient pass (include/quadgym.h, "teacher-student distillation"), written from the
formulae and their derivatives by hand, not from the kernel: the checker of tests/test_distill_reference.py (against torch float64
autograd) and tests/test_zz_distill_gpu.py.  NumPy; the torch statement of the same loss at the end imports torch when it is called."""
import collections
import math

import numpy as np

import policy_reference as R
import ppo_reference as G

STAT_NAMES = ("loss", "sq_err", "kl", "max_abs_err", "weight_sum")
MODES = ("mse", "kl")
WEIGHTS = ("none", "zeros", "frac")      # no weights; weights with exact zeros among them; fractional weights, none zero


def loss_and_grad(actor, log_std, critic, obs, target, out_tanh=False, mode="mse", coef=1.0, target_log_std=None, weights=None):
    """``(stats, grad)``: ``stats`` a dict over ``STAT_NAMES``, ``grad`` the float64 gradient of ``loss`` in the canonical flat order
    (zeros for the critic's entries, which the loss does not reach, and for ``log_std`` in MSE mode)."""
    B = len(obs)
    hs, mu = G._tower(actor, obs, out_tanh)
    w = np.ones(B) if weights is None else np.asarray(weights, np.float64)
    diff = mu - np.asarray(target, np.float64)
    sq = (diff ** 2).sum(-1)
    g_log_std = np.zeros(mu.shape[1])
    if mode == "mse":
        rows, dmean = sq, 2.0 * diff
    else:
        ls, lt = np.asarray(log_std, np.float64), np.asarray(target_log_std, np.float64)
        q = (np.exp(2.0 * lt) + diff ** 2) / np.exp(2.0 * ls)
        rows, dmean = (ls - lt + 0.5 * q - 0.5).sum(-1), diff / np.exp(2.0 * ls)
        g_log_std = coef / B * (w[:, None] * (1.0 - q)).sum(0)
    dmean = coef / B * w[:, None] * dmean
    if out_tanh:
        dmean = dmean * (1.0 - mu ** 2)
    g_actor = G._back(actor, hs, dmean)
    live = w != 0.0
    stats = {"loss": coef / B * np.sum(w * rows), "sq_err": np.sum(w * sq) / B, "kl": np.sum(w * rows) / B if mode == "kl" else 0.0,
             "max_abs_err": float(np.abs(diff[live]).max()) if live.any() else 0.0, "weight_sum": float(w.sum())}
    parts = [p.ravel() for Wb in g_actor for p in Wb] + [g_log_std] + [np.zeros(p.size) for Wb in (critic or []) for p in Wb]
    return stats, np.concatenate(parts)


def unflatten(flat, net, value):
    """``(actor, log_std, critic)`` as views of a canonical flat vector."""
    from quadruped_gym_amd.policy import FusedMlpPolicy
    layout = FusedMlpPolicy.param_layout(*net, value=value)

    def tower(name):
        return [tuple(flat[off:off + math.prod(shape)].reshape(shape) for off, shape in (layout[f"{name}.{k}.weight"], layout[f"{name}.{k}.bias"]))
                for k in range(len(net[1]) + 1)]
    off, shape = layout["log_std"]
    return tower("actor"), flat[off:off + shape[0]], tower("critic") if value else None


# ---- the cases of tests/test_zz_distill_gpu.py ---------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", ["net", "B", "out_tanh", "mode", "weights", "value", "seed"])
Data = collections.namedtuple("Data", ["actor", "log_std", "critic", "obs", "target", "target_log_std", "weights"])


def gradient_cases():
    """Every net of ``ppo_reference.NETS`` at every batch size of ``ppo_reference.BATCHES`` (the edges of a tile and of a slot); ``out_tanh``,
    the mode, the kind of weights and the critic vary along the list so that each combination of net and option, and of batch size and
    option, occurs (the weights go with (i + 2 j) mod 3, the critic with (i + j) mod 3: independent of each other).  Then the options
    in full on one net and batch, the critic alternating, and the wide net in both modes."""
    cases = []
    for i, net in enumerate(G.NETS):
        for j, B in enumerate(G.BATCHES):
            k = i + j
            cases.append(Case(net, B, bool(k % 2), MODES[(k // 2) % 2], WEIGHTS[(i + 2 * j) % 3], k % 3 != 0, 4000 + 10 * i + j))
    for out_tanh in (False, True):
        for mode in MODES:
            for weights in WEIGHTS:
                cases.append(Case(G.NETS[1], 600, out_tanh, mode, weights, len(cases) % 2 == 0, 5000 + len(cases)))
    cases += [Case(G.WIDE, 100, False, "mse", "zeros", True, 6000), Case(G.WIDE, 100, True, "kl", "frac", False, 6001)]
    return cases


def case_id(case):
    return "%d-%s-%d-B%d-tanh%d-%s-w%s-critic%d" % (case.net[0], "-".join(map(str, case.net[1])), case.net[2], case.B, case.out_tanh,
                                                    case.mode, case.weights, case.value)


def make_weights(rng, B, kind):
    """``none``: None; ``zeros``: U(0.5, 1.5) with about a third of the rows at exact zero (row 0 is kept: a batch of one row stays
    live); ``frac``: U(0.25, 1.75)."""
    if kind == "none":
        return None
    if kind == "frac":
        return rng.uniform(0.25, 1.75, B).astype(np.float32)
    w = rng.uniform(0.5, 1.5, B).astype(np.float32)
    dead = rng.random(B) < 1.0 / 3.0
    dead[0] = False
    w[dead] = 0.0
    return w


def make_data(rng, net, B, out_tanh, value, weights="none"):
    """A student and a teacher of the same shape (``ppo_reference.make_net``), observations with per-column scales 0.01 .. 10, the
    teacher's float32 means on them as targets, the teacher's ``log_std`` as ``target_log_std``."""
    actor, log_std, critic = G.make_net(rng, *net, value=value)
    teacher, teacher_log_std, _ = G.make_net(rng, *net, value=False)
    obs = (rng.standard_normal((B, net[0])) * np.logspace(-2, 1, net[0])).astype(np.float32)
    target = R.mlp(teacher, obs, out_tanh).astype(np.float32)
    return Data(actor, log_std, critic, obs, target, teacher_log_std, make_weights(rng, B, weights))


def build_case(case):
    """The ``Data`` of a case: seeded, so the CPU module and the GPU module see the same numbers."""
    return make_data(np.random.default_rng(case.seed), case.net, case.B, case.out_tanh, case.value, case.weights)


def kwargs(case, data, coef=0.7):
    """The keyword arguments of ``loss_and_grad`` / ``torch_gradients`` for a case (a coefficient other than 1, so that it shows)."""
    return dict(out_tanh=case.out_tanh, mode=case.mode, coef=coef, target_log_std=data.target_log_std if case.mode == "kl" else None,
                weights=data.weights)


# ---- the 20-step replay: distill_grad, then Adam, on one fixed batch (test_distill_reference.py asserts that it lowers sq_err) ---------------
REPLAY_NET, REPLAY_ROWS, REPLAY_STEPS, REPLAY_SEED, REPLAY_RATE = (33, (64, 64), 12), 512, 20, 77, float(np.float32(3e-3))


def replay_data():
    return make_data(np.random.default_rng(REPLAY_SEED), REPLAY_NET, REPLAY_ROWS, False, True)


# ---- the same loss in torch, for autograd -----------------------------------------------------------------------------------------------------
def torch_loss(mean, log_std_p, target, mode, coef, target_log_std=None, weights=None):
    """The loss of ``include/quadgym.h`` on the student's means ``mean [B, act_dim]`` as a torch expression (the KL term spelled out;
    tests/test_distill_reference.py holds it against ``torch.distributions.kl_divergence``)."""
    import torch
    diff = mean - target
    if mode == "mse":
        rows = (diff ** 2).sum(dim=1)
    else:
        rows = (log_std_p - target_log_std + (torch.exp(2 * target_log_std) + diff ** 2) / (2 * torch.exp(2 * log_std_p)) - 0.5).sum(dim=1)
    if weights is not None:
        rows = rows * weights
    return coef * rows.sum() / mean.shape[0]


def torch_gradients(data, out_tanh, mode, coef, target_log_std=None, weights=None, dtype=None, device="cpu"):
    """``(stats, [gradient per tensor in the canonical order])`` by autograd, as float64 NumPy arrays; ``dtype`` defaults to float64."""
    import torch
    import ppo_torch as T
    dtype = dtype or torch.float64

    def t(a):
        return None if a is None else torch.from_numpy(np.asarray(a)).to(dtype=dtype, device=device)
    actor_m = T.tower(data.actor, out_tanh, dtype, device)
    critic_m = T.tower(data.critic, False, dtype, device) if data.critic else None
    ls = torch.nn.Parameter(t(data.log_std))
    mean, target, w = actor_m(t(data.obs)), t(data.target), t(weights)
    total = torch_loss(mean, ls, target, mode, coef, t(target_log_std), w)
    total.backward()
    with torch.no_grad():
        diff = mean - target
        ww = torch.ones(len(data.obs), dtype=dtype, device=device) if w is None else w
        sq = (ww * (diff ** 2).sum(dim=1)).sum() / len(data.obs)
        live = ww != 0
        stats = {"loss": float(total), "sq_err": float(sq), "kl": float(total) / coef if mode == "kl" else 0.0,
                 "max_abs_err": float(diff[live].abs().max()) if bool(live.any()) else 0.0, "weight_sum": float(ww.sum())}
    tensors = list(actor_m.parameters()) + [ls] + (list(critic_m.parameters()) if critic_m else [])
    return stats, [(p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu().numpy().astype(np.float64) for p in tensors]
