"""The fused policy's backward passes and optimiser step over the shapes its ABI accepts: ``ppo_grad`` (csrc/qg_policy_grad.hip),
``distill_grad`` (csrc/qg_policy_distill.hip) and ``adam_step`` (csrc/qg_policy_opt.hip) on every row of tests/policy_reference.py's
SHAPE_TABLE, as tests/test_policy_shapes_gpu.py runs the forward pass on it.  tests/test_policy_backward_census.py says on the CPU which
shape classes of these kernels the table meets (all of tests/policy_backward_shapes.py's) and which the nets of tests/test_ppo_gpu.py,
tests/test_zz_distill_gpu.py and tests/test_zz_adam_gpu.py miss: the head lanes of actions 12..15, ``act_dim`` 16 and 4 k + 2,
``obs_dim`` 1 and 512, and every region boundary of the canonical vector that falls inside a thread's group of four in the Adam scatter.

Batches: 83 rows (five tiles and a three-row tail) for every row of the table; 513 (two slots) too for the rows that carry
``act_dim >= 13`` or 32 operand blocks.  ``out_tanh`` alternates along the table, value clipping in pairs; inputs are seeded per row,
made once and read-only.  The module captures no graph.

a. ``ppo_grad`` against ppo_reference.loss_and_grad by the rule of tests/test_ppo_gpu.py case 1: per parameter tensor
   max|g - g_ref| / max|g_ref| <= max(4 x torch float32 autograd on the GPU on the same inputs, 1e-6), statistics likewise in absolute
   terms, clip_fraction equal, all-zero references exact zeros, a wider row stride the same bits.
b. ``distill_grad`` against distill_reference.loss_and_grad by rule 1 of tests/test_zz_distill_gpu.py.
c. one live row gives the same bits at positions 0, 15, 16 and 82 where the fourth head quarter is live (``act_dim`` 15 and 16).
d. after two ``adam_step``s both operand images are what ``set_params`` would have packed: ``forward``, ``ppo_grad`` and
   ``distill_grad`` give the bits of a fresh handle -- every row, with and without a critic, with and without the transposed image.
e. one ``adam_step`` against float64 (adam_reference's tolerances, unchanged) on the rows that carry a new ``n_params % 4`` or a new
   boundary alignment.

With QG_BACKWARD_SHAPES_PARITY_OUT=<file> the cases of (a), (b) and (e) append their fused / torch / bound triples to that file
(profiles/r33/backward_shape_parity.txt).  Measured on an MI355X over the whole table, the worst ratio of a fused error to its bound:
``ppo_grad`` 0.56 (critic.1.bias, 65-16-16-16-2 at 83 rows; its statistics 0.11), ``distill_grad`` 0.68 (the kl statistic, 260-208-12;
its gradient 0.62, actor.2.bias of 257-112-224-1), ``adam_step`` 0.26 for m against the derived bound and 0.10 for v (p: 0.91, of
which half an ulp of p, its own rounding, is nearly all of the bound)."""
import collections
import functools
import math
import os

import numpy as np
import pytest
import torch

import adam_reference as A
import distill_reference as D
import policy_backward_shapes as S
import policy_reference as R
import ppo_reference as G
import ppo_torch as T
from policy_checks import DEV

from quadruped_gym_amd.policy import FusedMlpPolicy

pytestmark = pytest.mark.gpu
F32 = np.float32
Samples = collections.namedtuple("Samples", G.Batch._fields)
OLD_ADAM_NETS = [A.NETS[k] for k in "ABC"]


def _record(line):
    print(line)
    out = os.environ.get("QG_BACKWARD_SHAPES_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def _dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=DEV)          # a copy: the cached inputs are read-only


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _policy(desc, actor, log_std, critic, out_tanh, reserve):
    pol = FusedMlpPolicy(desc[0], desc[1], desc[2], out_tanh=out_tanh, value=critic is not None)
    pol.load_layers(actor, log_std, critic)
    if reserve:
        pol.reserve_grad(reserve)
    return pol


def _device_batch(batch, pad=0):
    """The batch as device tensors; ``pad`` > 0: the observations are the first columns of a wider buffer whose others hold 1e30."""
    obs = _dev(batch.observations)
    if pad:
        wide = torch.full((obs.shape[0], obs.shape[1] + pad), 1.0e30, device=DEV)
        wide[:, :obs.shape[1]] = obs
        obs = wide[:, :batch.observations.shape[1]]
        assert obs.stride() == (batch.observations.shape[1] + pad, 1)
    return Samples(obs, _dev(batch.actions), _dev(batch.old_values), _dev(batch.old_log_prob), _dev(batch.advantages), _dev(batch.returns))


def _ppo(pol, dbatch, **kw):
    grad = torch.full((pol.n_params,), float("nan"), device=DEV)
    stats = torch.full((8,), float("nan"), device=DEV)
    pol.ppo_grad(dbatch, grad, stats, **kw)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), stats.cpu().numpy()


def _distill(pol, obs, target, mode="mse", coef=1.0, target_log_std=None, weights=None):
    grad = torch.full((pol.n_params,), float("nan"), device=DEV)
    stats = torch.full((8,), float("nan"), device=DEV)
    pol.distill_grad(obs, target, grad, stats, loss=mode, coef=coef, target_log_std=target_log_std, weights=weights)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), stats.cpu().numpy()


def test_batch_sizes_come_from_the_kernels_partition():
    assert (G.TILE_ROWS, G.SLOT_ROWS) == (FusedMlpPolicy.GRAD_TILE_ROWS, FusedMlpPolicy.GRAD_SLOT_ROWS)
    assert S.B_SMALL == 5 * G.TILE_ROWS + 3 and S.B_TWO_SLOTS == G.SLOT_ROWS + 1 and S.ADAM_SLOT == FusedMlpPolicy.ADAM_SLOT


# ---- a. ppo_grad against the float64 reference ---------------------------------------------------------------------------------------
PPO_KW = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5)


@functools.lru_cache(maxsize=None)
def _ppo_reference(case):
    actor, log_std, critic, batch = S.build_ppo_case(case)
    stats, grad = G.loss_and_grad(actor, log_std, critic, batch, case.out_tanh, clip_range_vf=case.clip_range_vf, **PPO_KW)
    grad.setflags(write=False)
    return stats, grad


@pytest.mark.parametrize("case", S.ppo_cases(), ids=G.case_id)
def test_ppo_gradient_and_statistics_match_float64_reference(case):
    actor, log_std, critic, batch = S.build_ppo_case(case)
    ref_stats, ref_grad = _ppo_reference(case)
    kw = dict(clip_range_vf=case.clip_range_vf, **PPO_KW)
    t_stats, t_grads = T.gradients(actor, log_std, critic, batch, case.out_tanh, 0.2, case.clip_range_vf, 0.01, 0.5, torch.float32, DEV)
    layout = FusedMlpPolicy.param_layout(*case.net, value=case.value)
    pol = _policy(case.net, actor, log_std, critic, case.out_tanh, case.B)
    assert list(pol.param_slices().items()) == list(layout.items()) and len(t_grads) == len(layout)
    outs = []
    for name_l, pad in (("contiguous", 0), ("strided", 1)):
        grad, stats = _ppo(pol, _device_batch(batch, pad), **kw)
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
            lines.append(f"{name}: fused {err:.3e} torch {terr:.3e} bound {bound:.3e} ratio {err / bound:.2f}")
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
            lines.append(f"{name}: fused {err:.3e} torch {terr:.3e} bound {bound:.3e} ratio {err / bound:.2f}")
            if not err <= bound:
                failures.append((name, err, terr))
        _record(f"ppo {G.case_id(case)} obs={name_l}: " + "  ".join(lines))
        assert not failures, failures
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and np.array_equal(_bits(outs[0][1]), _bits(outs[1][1]))     # the row stride
    pol.close()


# ---- b. distill_grad against the float64 reference -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _distill_reference(case):
    data = S.distill_data(case.i, case.B)
    stats, grad = D.loss_and_grad(data.actor, data.log_std, data.critic, data.obs, data.target, **S.distill_kwargs(case))
    grad.setflags(write=False)
    return stats, grad


def _distill_audit(layout, grad, stats, ref_grad, ref_stats, t_grads, t_stats):
    """Rule 1 of tests/test_zz_distill_gpu.py: ``(lines, failures)``."""
    lines, failures = [], []
    if not (np.isfinite(grad).all() and np.isfinite(stats).all() and not stats[5:].any()):
        failures.append(("not finite, or stats[5:] not zero",))
    for (name, (off, shape)), tg in zip(layout.items(), t_grads):
        n = math.prod(shape)
        ref, got = ref_grad[off:off + n], grad[off:off + n]
        scale = np.abs(ref).max()
        if scale == 0.0:
            lines.append(f"{name}: reference all zeros")
            if _bits(got).any():
                failures.append((name, "not exact +0.0"))
            continue
        err, terr = np.abs(got.astype(np.float64) - ref).max() / scale, np.abs(tg.ravel() - ref).max() / scale
        bound = max(4.0 * terr, 1e-6)
        lines.append(f"{name}: fused {err:.3e} torch {terr:.3e} bound {bound:.3e} ratio {err / bound:.2f}")
        if not err <= bound:
            failures.append((name, err, terr))
    for k, name in enumerate(D.STAT_NAMES):
        err, terr = abs(float(stats[k]) - ref_stats[name]), abs(t_stats[name] - ref_stats[name])
        bound = float(np.spacing(np.float32(abs(ref_stats[name])))) if name == "weight_sum" else max(4.0 * terr, 1e-6)
        lines.append(f"{name}: fused {err:.3e} torch {terr:.3e} bound {bound:.3e} ratio {err / bound:.2f}")
        if not err <= bound:
            failures.append((name, err, terr))
    return lines, failures


@pytest.mark.parametrize("case", S.distill_cases(), ids=S.distill_id)
def test_distill_gradient_and_statistics_match_float64_reference(case):
    desc, data, kw = R.SHAPE_TABLE[case.i], S.distill_data(case.i, case.B), S.distill_kwargs(case)
    ref_stats, ref_grad = _distill_reference(case)
    t_stats, t_grads = D.torch_gradients(data, dtype=torch.float32, device=DEV, **kw)
    layout = FusedMlpPolicy.param_layout(*desc, value=True)
    pol = _policy(desc, data.actor, data.log_std, data.critic, kw["out_tanh"], case.B)
    grad, stats = _distill(pol, _dev(data.obs), _dev(data.target), case.mode, kw["coef"], _dev(kw["target_log_std"]), _dev(kw["weights"]))
    lines, failures = _distill_audit(layout, grad, stats, ref_grad, ref_stats, t_grads, t_stats)
    _record(f"distill {S.distill_id(case)}: " + "  ".join(lines))
    assert not failures, failures
    assert (stats[2] == 0.0) == (case.mode == "mse")
    if case.weights == "zeros":
        assert kw["weights"][0] != 0 and np.count_nonzero(kw["weights"] == 0) > 0
    pol.close()


# ---- c. one live row, any position, same bits: the fourth head quarter -----------------------------------------------------------------
def _moved(B, pos):
    """Base row 0 at position ``pos``, the others in their order."""
    return np.r_[1:pos + 1, 0, pos + 1:B]


@pytest.mark.parametrize("i", S.PLACEMENT_ROWS, ids=S.row_id)
def test_one_live_ppo_row_gives_the_same_bits_at_any_position(i):
    desc, B, tanh = R.SHAPE_TABLE[i], S.B_SMALL, S.out_tanh(i)
    rng = np.random.default_rng(9000 + i)
    actor, log_std, critic = G.make_net(rng, *desc)
    base = G.make_batch(rng, actor, log_std, critic, tanh, B)
    ratio = G.row_terms(actor, log_std, critic, base, tanh)[1]
    j = int(np.argmax(np.abs(ratio - 1.0) < 0.1))        # a row well inside the clip range becomes row 0, the live one
    assert abs(ratio[j] - 1.0) < 0.1
    swap = np.arange(B)
    swap[[0, j]] = [j, 0]
    base = G.Batch(*(a[swap] for a in base))
    pol = _policy(desc, actor, log_std, critic, tanh, B)
    grads = []
    for pos in S.POSITIONS:
        adv = np.zeros(B, np.float32)
        adv[pos] = 0.75
        b = G.Batch(*(a[_moved(B, pos)] for a in base))._replace(advantages=adv)
        assert np.array_equal(b.observations[pos], base.observations[0])
        grads.append(_ppo(pol, _device_batch(b), ent_coef=0.0, vf_coef=0.0)[0])
    slices = pol.param_slices()
    last = len(desc[1])
    for name in ("actor.0.weight", f"actor.{last}.weight", f"actor.{last}.bias", "log_std"):      # the row is not clipped: a gradient in
        off, shape = slices[name]                                                                  # every action's row, 12..15 included
        g = grads[0][off:off + math.prod(shape)].reshape(shape[0], -1)
        assert np.all(np.abs(g).max(axis=1) > 0), name
    assert not grads[0][slices["critic.0.weight"][0]:].any()                                       # vf_coef = 0
    for g in grads[1:]:
        assert np.array_equal(_bits(grads[0]), _bits(g))
    pol.close()


@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("i", S.PLACEMENT_ROWS, ids=S.row_id)
def test_one_live_distill_row_gives_the_same_bits_at_any_position(i, mode):
    desc, B, tanh = R.SHAPE_TABLE[i], S.B_SMALL, S.out_tanh(i)
    data = S.distill_data(i, B)
    pol = _policy(desc, data.actor, data.log_std, data.critic, tanh, B)
    lt = _dev(data.target_log_std) if mode == "kl" else None
    outs = []
    for pos in S.POSITIONS:
        order = _moved(B, pos)
        w = np.zeros(B, np.float32)
        w[pos] = 0.75
        outs.append(_distill(pol, _dev(data.obs[order]), _dev(data.target[order]), mode, 1.0, lt, _dev(w)))
    grad, stats = outs[0]
    slices = pol.param_slices()
    last = len(desc[1])
    for name in ("actor.0.weight", f"actor.{last}.weight", f"actor.{last}.bias") + (("log_std",) if mode == "kl" else ()):
        off, shape = slices[name]
        assert np.all(np.abs(grad[off:off + math.prod(shape)].reshape(shape[0], -1)).max(axis=1) > 0), name
    assert stats[4] == np.float32(0.75) and stats[3] > 0 and not _bits(grad[slices["critic.0.weight"][0]:]).any()
    for g, s in outs[1:]:
        assert np.array_equal(_bits(g), _bits(grad)) and np.array_equal(_bits(s), _bits(stats))
    pol.close()


# ---- d. the Adam step's operand images --------------------------------------------------------------------------------------------------
def _adam_policy(desc, params, grad_rows, adam):
    obs_dim, hidden, act_dim, critic = desc
    pol = FusedMlpPolicy(obs_dim, hidden, act_dim, out_tanh=False, value=critic)
    assert pol.n_params == A.n_params(desc) == S.n_params(desc[:3], critic)
    pol.set_params(params)
    if grad_rows:
        pol.reserve_grad(grad_rows)
    if adam:
        pol.reserve_adam()
    return pol


def _outputs(pol, obs, eps, batch, target, target_log_std):
    """The bits of everything that reads an operand image: forward (action, log-prob, value), and with ``batch`` both gradient passes."""
    n = obs.shape[0]
    acts, lp = torch.full((n, pol.act_dim), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
    val = torch.full((n,), float("nan"), device=DEV) if pol.has_value else None
    pol.forward(obs, acts, eps=eps, log_prob=lp, value=val)
    outs = [acts, lp] + ([val] if val is not None else [])
    if batch is not None:
        for _ in range(2):
            outs += [torch.full((pol.n_params,), float("nan"), device=DEV), torch.full((8,), float("nan"), device=DEV)]
        pol.ppo_grad(batch, outs[-4], outs[-3], clip_range_vf=0.3 if pol.has_value else None, ent_coef=0.01)
        pol.distill_grad(obs, target, outs[-2], outs[-1], loss="kl", target_log_std=target_log_std)
    torch.cuda.synchronize()
    outs = [o.cpu().numpy() for o in outs]
    assert all(np.isfinite(o).all() for o in outs)
    return [_bits(o) for o in outs]


@pytest.mark.parametrize("with_grad", [True, False], ids=["reserve_grad", "forward_only"])
@pytest.mark.parametrize("critic", [True, False], ids=["critic", "actor_only"])
@pytest.mark.parametrize("i", S.TABLE, ids=S.row_id)
def test_images_after_adam_steps_are_what_set_params_would_have_packed(i, critic, with_grad):
    rows = S.B_SMALL
    desc = S.adam_desc(i, critic)
    obs_dim, _, act_dim, _ = desc
    pol = _adam_policy(desc, A.initial_params(desc), rows if with_grad else 0, True)
    gen = torch.Generator(device=DEV).manual_seed(3 + i)
    obs, eps, target = (torch.randn(s, device=DEV, generator=gen) for s in ((rows, obs_dim), (rows, act_dim), (rows, act_dim)))
    lt = torch.full((act_dim,), -1.0, device=DEV)
    batch = None
    if with_grad:
        acts, lp = torch.empty((rows, act_dim), device=DEV), torch.empty(rows, device=DEV)
        val = torch.empty(rows, device=DEV) if critic else None
        pol.forward(obs, acts, eps=eps, log_prob=lp, value=val)
        batch = Samples(obs, acts, val, lp, torch.randn(rows, device=DEV, generator=gen),
                        torch.randn(rows, device=DEV, generator=gen) if critic else None)
    before = _outputs(pol, obs, eps, batch, target, lt)
    out = torch.full((pol.n_params,), float("nan"), device=DEV)
    for k in range(2):                                   # a rate that moves the parameters by a visible amount
        pol.adam_step(_dev(A.make_gradient(desc, 40 + k, 1.0)), lr=1e-3, params_out=out)
    after = _outputs(pol, obs, eps, batch, target, lt)
    assert all(not np.array_equal(a, b) for a, b in zip(before, after))
    params = pol.params()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(params)) and np.abs(params - A.initial_params(desc)).max() > 0.5e-3
    fresh = _adam_policy(desc, params, rows if with_grad else 0, False)
    want = _outputs(fresh, obs, eps, batch, target, lt)
    assert len(want) == (2 + int(critic)) + (4 if with_grad else 0)
    for k, (a, b) in enumerate(zip(after, want)):
        assert np.array_equal(a, b), (k, int(np.count_nonzero(a != b)))
    fresh.close()
    pol.close()


# ---- e. one Adam step against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,critic", S.adam_float64_rows(OLD_ADAM_NETS), ids=lambda v: S.row_id(v) if not isinstance(v, bool) else f"critic{int(v)}")
def test_one_adam_step_matches_float64(i, critic):
    desc, t, mode = S.adam_desc(i, critic), 1, "active"
    p, m, v, g, max_norm, ref = A.one_step_case(desc, t, mode)
    p64, m64, v64, info = ref
    pol = _adam_policy(desc, p, 0, True)
    pol.load_adam_state({"step": t - 1, "exp_avg": m, "exp_avg_sq": v})
    grad, out, stats = _dev(g), torch.full((pol.n_params,), float("nan"), device=DEV), torch.full((4,), float("nan"), device=DEV)
    pol.adam_step(grad, lr=A.LR, betas=(A.BETA1, A.BETA2), eps=A.EPS, max_grad_norm=max_norm, params_out=out, stats=stats)
    torch.cuda.synchronize()
    st = pol.adam_state()
    gp, gm, gv, gt = pol.params(), st["exp_avg"], st["exp_avg_sq"], st["step"]
    stats = stats.cpu().numpy()
    assert torch.equal(grad, _dev(g))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(gp)) and gt == t
    tp, tm, tv = A.gpu_tolerances(p64, m64, v64)
    derived = A.derived_m_tolerance(m, g, float(info["coef"]), m64)
    errs = [np.abs(got.astype(np.float64) - want) for got, want in ((gp, p64), (gm, m64), (gv, v64))]
    dev = A.deviations(gm, gv, (p.astype(np.float64) - gp.astype(np.float64)), ref)
    worst = [int(np.argmax(e / tol)) for e, tol in zip(errs, (tp, tm, tv))]             # p's bound is mostly half an ulp of p, its own rounding
    _record(f"adam {S.row_id(i)} critic {int(critic)} n_params {pol.n_params} t {t} {mode}: m {dev[0]:.3f} ulp  v {dev[1]:.3f} ulp  " +
            "  ".join(f"{name}: fused {e[k]:.3e} bound {tol[k]:.3e} ratio {e[k] / tol[k]:.2g}"
                      for name, e, tol, k in zip("pmv", errs, (tp, tm, tv), worst)) +
            f"  m against the derived bound: ratio {np.max(errs[1] / derived):.2f}")
    assert np.all(errs[0] <= tp) and np.all(errs[1] <= tm) and np.all(errs[2] <= tv)
    assert np.all(errs[1] <= derived)
    # stats: norm before clipping, coef, t, lr -- the rule of tests/test_zz_adam_gpu.py::test_one_step_matches_float64
    assert abs(float(stats[0]) - float(info["norm"])) <= float(A.ulp32(info["norm"]))
    want_coef = min(F32(1.0), F32(max_norm) / (stats[0] + F32(1e-6)))
    assert stats[1] == want_coef and stats[1] < 1.0
    assert abs(float(stats[1]) - float(info["coef"])) <= 2 * float(A.ulp32(info["coef"]))
    assert stats[2] == t and stats[3] == F32(A.LR)
    pol.close()
