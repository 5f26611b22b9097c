"""FusedMlpPolicy.distill_grad on the GPU (qg_policy_distill_grad_device, csrc/qg_policy_distill.hip) against the float64 checker of
tests/distill_reference.py.

Tolerance (rule 1): no fixed figure -- the rule of tests/test_ppo_gpu.py.  Per parameter tensor err = max|g - g_ref| / max|g_ref|; the same
quantity is computed for torch float32 autograd ON THE GPU on the same inputs -- the path the pass replaces -- and the pass may have at
most max(4 x torch's, 1e-6).  The same with absolute errors for loss, sq_err, kl and max_abs_err; weight_sum within one float32 ulp of
the float64 sum.  A tensor whose reference gradient is all zeros (the critic; log_std in MSE mode) must be exact zeros, sign bit clear.
With QG_DISTILL_PARITY_OUT=<file> every case appends both paths' maxima to that file (profiles/r29/distill_parity.txt).

Placement of live rows (case 3).  The sum over the rows is defined with its grouping (include/quadgym.h): a tile's 16 rows are one
float32 chain in ascending row order, tiles are added in float64.  A row of weight zero adds exact zeros, so ONE live row may sit
anywhere, and SEVERAL give the same bits wherever they sit as long as their order and their grouping into tiles are the same: all in
one tile (at any offsets, in any tile, the ragged last one included), or each in a tile of its own.  Between the two groupings the sums
are different sums, and the last bit may differ; that is not asserted either way.

The module's name puts it behind the other modules in collection, as the others that capture hipGraphs."""
import collections
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import adam_reference as A
import distill_reference as D
import policy_reference as R
import ppo_reference as G
from helpers import capture_graph
from policy_checks import DEV

from quadruped_gym_amd import _abi
from quadruped_gym_amd.policy import FusedMlpPolicy, QgDistillBatch, QgDistillParams

pytestmark = pytest.mark.gpu
Samples = collections.namedtuple("Samples", G.Batch._fields)


def _record(line):
    print(line)
    out = os.environ.get("QG_DISTILL_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _policy(net, data, out_tanh, reserve, adam=False):
    pol = FusedMlpPolicy(net[0], net[1], net[2], out_tanh=out_tanh, value=data.critic is not None)
    pol.load_layers(data.actor, data.log_std, data.critic)
    if reserve:
        pol.reserve_grad(reserve)
    if adam:
        pol.reserve_adam()
    return pol


def _run(pol, obs, target, mode="mse", coef=1.0, target_log_std=None, weights=None):
    """One call on NaN-filled outputs: ``(grad, stats)`` as NumPy."""
    grad = torch.full((pol.n_params,), float("nan"), device=DEV)
    stats = torch.full((8,), float("nan"), device=DEV)
    pol.distill_grad(obs, target, grad, stats, loss=mode, coef=coef, target_log_std=target_log_std, weights=weights)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), stats.cpu().numpy()


def _audit(layout, grad, stats, ref_grad, ref_stats, t_grads, t_stats):
    """Rule 1: ``(lines, failures)``."""
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
        lines.append(f"{name}: fused {err:.3e} torch {terr:.3e} bound {bound:.3e}")
        if not err <= bound:
            failures.append((name, err, terr))
    for k, name in enumerate(D.STAT_NAMES):
        err, terr = abs(float(stats[k]) - ref_stats[name]), abs(t_stats[name] - ref_stats[name])
        bound = float(np.spacing(np.float32(abs(ref_stats[name])))) if name == "weight_sum" else max(4.0 * terr, 1e-6)
        lines.append(f"{name}: fused {err:.3e} torch {terr:.3e} bound {bound:.3e}")
        if not err <= bound:
            failures.append((name, err, terr))
    return lines, failures


def _torch32(data, **kw):
    return D.torch_gradients(data, dtype=torch.float32, device=DEV, **kw)


# ---- 1. gradient and statistics against the float64 reference -------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.gradient_cases(), ids=D.case_id)
def test_gradient_and_statistics_match_float64_reference(case):
    data = D.build_case(case)
    kw = D.kwargs(case, data)
    ref_stats, ref_grad = D.loss_and_grad(data.actor, data.log_std, data.critic, data.obs, data.target, **kw)
    t_stats, t_grads = _torch32(data, **kw)
    layout = FusedMlpPolicy.param_layout(*case.net, value=case.value)
    pol = _policy(case.net, data, case.out_tanh, case.B)
    grad, stats = _run(pol, _dev(data.obs), _dev(data.target), case.mode, kw["coef"], _dev(kw["target_log_std"]), _dev(data.weights))
    lines, failures = _audit(layout, grad, stats, ref_grad, ref_stats, t_grads, t_stats)
    _record(f"{D.case_id(case)}: " + "  ".join(lines))
    assert not failures, failures
    assert (stats[2] == 0.0) == (case.mode == "mse")
    pol.close()


# ---- 2. the row stride changes nothing --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in D.gradient_cases() if c.B in (17, 513)][::3], ids=D.case_id)
def test_rows_inside_a_wider_buffer_give_the_same_bits(case):
    data = D.build_case(case)
    kw = D.kwargs(case, data)
    pol = _policy(case.net, data, case.out_tanh, case.B)
    args = (_dev(data.target), case.mode, kw["coef"], _dev(kw["target_log_std"]), _dev(data.weights))
    obs = _dev(data.obs)
    want = _run(pol, obs, *args)
    wide = torch.full((case.B, case.net[0] + 5), 1.0e30, device=DEV)
    wide[:, :case.net[0]] = obs
    for rows in (wide[:, :case.net[0]], wide):                 # the actor's slice of the wide rows, and the wide rows themselves
        got = _run(pol, rows, *args)
        assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    pol.close()


# ---- 3. live rows among rows of weight zero ---------------------------------------------------------------------------------------------
PLACEMENTS = {
    1: [[(0,), (15,), (16,), (99,)]],
    # all in one tile: the first, at other offsets, another tile, the ragged last tile -- and each in a tile of its own
    3: [[(0, 1, 2), (3, 9, 15), (16, 20, 31), (96, 97, 99)], [(0, 16, 32), (15, 47, 99), (5, 40, 98)]],
}


@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("k", sorted(PLACEMENTS))
def test_live_rows_give_the_same_bits_wherever_they_sit(k, mode):
    net, B = (33, (64, 64), 12), 100
    data = D.make_data(np.random.default_rng(41 + k), net, B, True, True)
    pol = _policy(net, data, True, B)
    lt = _dev(data.target_log_std) if mode == "kl" else None
    for group in PLACEMENTS[k]:
        outs = []
        for pos in group:
            order = np.empty(B, np.int64)                       # base rows 0 .. k - 1 go to `pos`, the others fill the rest in order
            order[list(pos)] = np.arange(k)
            order[np.setdiff1d(np.arange(B), pos)] = np.arange(k, B)
            w = np.zeros(B, np.float32)
            w[list(pos)] = (0.75, 1.5, 1.0)[:k]
            outs.append(_run(pol, _dev(data.obs[order]), _dev(data.target[order]), mode, 1.0, lt, _dev(w)))
        grad, stats = outs[0]
        lo, shape = pol.param_slices()["actor.0.weight"]
        assert np.abs(grad[lo:lo + math.prod(shape)]).max() > 0 and stats[4] == np.float32(sum((0.75, 1.5, 1.0)[:k])) and stats[3] > 0
        assert not _bits(grad[pol.param_slices()["critic.0.weight"][0]:]).any()
        for g, s in outs[1:]:
            assert np.array_equal(_bits(g), _bits(grad)) and np.array_equal(_bits(s), _bits(stats)), group
    pol.close()


# ---- 4. reproducible: eager steps and the replays of a captured step ------------------------------------------------------------------------
def test_three_replays_of_a_captured_step_leave_the_bits_of_three_eager_steps():
    data = D.replay_data()
    obs, target, lt = _dev(data.obs), _dev(data.target), _dev(data.target_log_std)
    w = _dev(D.make_weights(np.random.default_rng(5), D.REPLAY_ROWS, "zeros"))
    kw = dict(loss="kl", coef=0.5, target_log_std=lt, weights=w)
    eager, pol = (_policy(D.REPLAY_NET, data, False, D.REPLAY_ROWS, adam=True) for _ in range(2))
    grad, stats = torch.zeros(pol.n_params, device=DEV), torch.zeros(8, device=DEV)
    want = []
    for _ in range(3):
        eager.distill_grad(obs, target, grad, stats, **kw)
        eager.adam_step(grad, lr=D.REPLAY_RATE)
        torch.cuda.synchronize()
        want.append((eager.params(), grad.cpu().numpy(), stats.cpu().numpy()))
    fresh = _policy(D.REPLAY_NET, data, False, D.REPLAY_ROWS)
    second = _run(fresh, obs, target, "kl", 0.5, lt, w)
    fresh.close()
    assert np.array_equal(_bits(second[0]), _bits(want[0][1])) and np.array_equal(_bits(second[1]), _bits(want[0][2]))   # two runs, same bits
    grad.fill_(float("nan")), stats.fill_(float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with capture_graph(graph, DEV):
        pol.distill_grad(obs, target, grad, stats, **kw)
        pol.adam_step(grad, lr=D.REPLAY_RATE)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(pol.params()), _bits(R.flatten(data.actor, data.log_std, data.critic)))                # a capture runs nothing
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = (pol.params(), grad.cpu().numpy(), stats.cpu().numpy())
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want[k])), k
    assert not np.array_equal(_bits(want[0][0]), _bits(want[2][0]))
    del graph
    eager.close(), pol.close()


# ---- 5. the neighbours on the handle -----------------------------------------------------------------------------------------------------------
def test_ppo_grad_and_forward_are_undisturbed():
    net, B = (33, (64, 64), 12), 600
    rng = np.random.default_rng(43)
    data = D.make_data(rng, net, B, False, True, "frac")
    batch = G.make_batch(rng, data.actor, data.log_std, data.critic, False, B, 0.2, 0.3)     # (its own observations; any targets will do)
    pol = _policy(net, data, False, B)
    db = Samples(*(_dev(a) for a in batch))
    acts, lp, val = torch.empty((B, 12), device=DEV), torch.empty(B, device=DEV), torch.empty(B, device=DEV)
    eps = _dev(rng.standard_normal((B, 12)).astype(np.float32))

    def ppo():
        grad, stats = torch.full((pol.n_params,), float("nan"), device=DEV), torch.full((8,), float("nan"), device=DEV)
        pol.ppo_grad(db, grad, stats, clip_range_vf=0.3, ent_coef=0.01)
        pol.forward(db.observations, acts, eps=eps, log_prob=lp, value=val)
        torch.cuda.synchronize()
        return [_bits(t.cpu().numpy()) for t in (grad, stats, acts, lp, val)]
    before, params = ppo(), pol.params()
    for mode in D.MODES:
        grad, stats = _run(pol, db.observations, _dev(data.target), mode, 1.0, _dev(data.target_log_std), _dev(data.weights))
        assert np.isfinite(grad).all() and np.abs(grad).max() > 0
        assert np.array_equal(_bits(pol.params()), _bits(params))
        assert all(np.array_equal(a, b) for a, b in zip(before, ppo())), mode
    pol.close()


# ---- 6. the 20-step replay of tests/test_distill_reference.py ------------------------------------------------------------------------------------
def test_twenty_steps_of_distill_grad_and_adam_step():
    data = D.replay_data()
    obs, target = _dev(data.obs), _dev(data.target)
    pol = _policy(D.REPLAY_NET, data, False, D.REPLAY_ROWS, adam=True)
    n, K = pol.n_params, D.REPLAY_STEPS
    grads, stats, params_out = torch.zeros((K + 1, n), device=DEV), torch.zeros((K + 1, 8), device=DEV), torch.zeros((K, n), device=DEV)
    for s in range(K + 1):
        pol.distill_grad(obs, target, grads[s], stats[s])
        if s < K:
            pol.adam_step(grads[s], lr=D.REPLAY_RATE, params_out=params_out[s])
    torch.cuda.synchronize()
    grads, stats, params_out = grads.cpu().numpy(), stats.cpu().numpy(), params_out.cpu().numpy()
    assert np.array_equal(_bits(pol.params()), _bits(params_out[-1]))
    layout = FusedMlpPolicy.param_layout(*D.REPLAY_NET, value=True)
    flat = R.flatten(data.actor, data.log_std, data.critic)
    for s in range(K + 1):                                      # step s was taken at the parameters step s - 1 recorded
        actor, log_std, critic = D.unflatten(flat if s == 0 else params_out[s - 1], D.REPLAY_NET, True)
        at = data._replace(actor=actor, log_std=log_std, critic=critic)
        ref_stats, ref_grad = D.loss_and_grad(actor, log_std, critic, data.obs, data.target)
        t_stats, t_grads = _torch32(at, out_tanh=False, mode="mse", coef=1.0)
        lines, failures = _audit(layout, grads[s], stats[s], ref_grad, ref_stats, t_grads, t_stats)
        assert not failures, (s, failures)
    print("sq_err on the device:", " ".join(f"{e:.4f}" for e in stats[:, 1]))
    assert stats[-1, 1] < stats[0, 1]
    pol.close()


# ---- 7. the public recipe, small -------------------------------------------------------------------------------------
def test_dagger_recipe_on_the_wide_row():
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
    from quadruped_gym_amd.privileged import DevicePrivilegedVecEnv
    from quadruped_gym_amd.rollout import DeviceRolloutBuffer
    N, K, ACT, hidden = 64, 8, 12, (64, 64)
    env = DevicePrivilegedVecEnv(POWalkingQuadrupedVecEnv(N, obs_window=2, max_time=0.02, nan_direction=False, random_controls=True,
                                                          device_commands=True), force_threshold=1.0)
    O, W = env.actor_obs_dim, env.obs_dim
    rng = np.random.default_rng(44)
    t_actor, t_log_std, _ = G.make_net(rng, W, hidden, ACT, value=False)
    s_actor, s_log_std, _ = G.make_net(rng, O, hidden, ACT, value=False)
    teacher, student = FusedMlpPolicy(W, hidden, ACT, value=False), FusedMlpPolicy(O, hidden, ACT, value=False)
    teacher.load_layers(t_actor, t_log_std), student.load_layers(s_actor, s_log_std)
    student.reserve_grad(N * K // 2), student.reserve_adam()
    buf = DeviceRolloutBuffer(N, K, W, ACT)
    z = lambda *s, **kw: torch.zeros(s, device=DEV, **kw)
    cur, nxt, actions, logp, value, reward, done = z(N, W), z(N, W), z(N, ACT), z(N), z(N), z(N), z(N, dtype=torch.uint8)
    eps = torch.randn((K, N, ACT), device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    cur.copy_(torch.from_numpy(env.reset()).to(DEV))
    buf.begin(cur)
    for t in range(K):                                          # the STUDENT acts, on the actor's window of the wide row
        student.forward(cur[:, :O], actions, eps=eps[t], log_prob=logp)
        env.step_tensor(actions, nxt, reward, done)
        buf.add(nxt, actions, logp, value, reward, done)
        cur.copy_(nxt)
    buf.compute_returns_and_advantage(value)
    torch.cuda.synchronize()
    rows_before, teacher_before = buf.observations.clone(), teacher.params()
    idx = torch.randperm(N * K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    B = N * K // 2
    target, grad, stats, params_out = z(B, ACT), z(student.n_params), z(8), z(student.n_params)
    lt = _dev(t_log_std)
    layout, flat = student.param_slices(), student.params()
    for half, mode in enumerate(D.MODES):
        batch = buf.sample(idx[half * B:(half + 1) * B].contiguous())
        teacher.forward(batch.observations, target)             # the labels: the teacher's means on the whole wide rows
        student.distill_grad(batch.observations, target, grad, stats, loss=mode, target_log_std=lt if mode == "kl" else None)
        student.adam_step(grad, lr=1e-3, params_out=params_out)
        torch.cuda.synchronize()
        rows, labels = batch.observations.cpu().numpy(), target.cpu().numpy()
        assert np.isfinite(labels).all() and np.abs(labels).max() > 0
        actor, log_std, _ = D.unflatten(flat, (O, hidden, ACT), False)
        at = D.Data(actor, log_std, None, np.ascontiguousarray(rows[:, :O]), labels, t_log_std, None)
        kw = dict(out_tanh=False, mode=mode, coef=1.0, target_log_std=t_log_std if mode == "kl" else None)
        ref_stats, ref_grad = D.loss_and_grad(actor, log_std, None, at.obs, labels, **kw)
        t_stats, t_grads = _torch32(at, **kw)
        lines, failures = _audit(layout, grad.cpu().numpy(), stats.cpu().numpy(), ref_grad, ref_stats, t_grads, t_stats)
        assert not failures, (mode, failures)
        flat = params_out.cpu().numpy()
        assert np.array_equal(_bits(flat), _bits(student.params())) and stats[1] > 0
    assert torch.equal(buf.observations, rows_before) and np.array_equal(_bits(teacher.params()), _bits(teacher_before))
    assert np.isfinite(rows_before.cpu().numpy()).all()
    teacher.close(), student.close(), buf.close(), env.close()


# ---- 8. refusals that need a handle --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    net, B = (33, (64, 64), 12), 64
    data = D.make_data(np.random.default_rng(45), net, B, False, True)
    pol = _policy(net, data, False, 0)
    obs, target = _dev(data.obs), _dev(data.target)
    grad, stats = torch.full((pol.n_params,), 7.0, device=DEV), torch.full((8,), 7.0, device=DEV)
    with pytest.raises(_abi.QuadGymError, match="reserved 0 rows"):
        pol.distill_grad(obs, target, grad, stats)               # nothing reserved
    pol.reserve_grad(B - 1)
    with pytest.raises(_abi.QuadGymError, match="reserved 63 rows"):
        pol.distill_grad(obs, target, grad, stats)               # B > the rows reserved
    pol.reserve_grad(B)
    lib, buf = _abi.load_library(), _dev(np.zeros(64, np.float32))
    p = QgDistillParams.make()
    b = QgDistillBatch.make(32, obs=obs.data_ptr(), target_mean=target.data_ptr())
    assert lib.qg_policy_distill_grad_device(pol._h, C.byref(p), B, C.byref(b), grad.data_ptr(), None, None) == -1
    assert b"obs_stride 32 < obs_dim 33" in lib.qg_last_error()
    for bad in (dict(loss="kl"), dict(coef=float("inf")), dict(loss="l1")):
        with pytest.raises(ValueError):
            pol.distill_grad(obs, target, grad, stats, **bad)
    for bad in (dict(grad=grad.double()), dict(grad=grad[:-1]), dict(grad=grad.cpu()), dict(target_mean=target[:, :-1].contiguous()),
                dict(weights=buf[:B - 1]), dict(obs=obs[:, :-1]), dict(stats=stats[:4])):
        args = dict(obs=obs, target_mean=target, grad=grad, stats=stats)
        args.update(bad)
        with pytest.raises(ValueError):
            pol.distill_grad(**args)
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all()) and bool((stats == 7.0).all())          # nothing was launched
    pol.distill_grad(obs, target, grad, None)                                # stats are optional
    torch.cuda.synchronize()
    assert torch.isfinite(grad).all() and bool((stats == 7.0).all())
    pol.close()
