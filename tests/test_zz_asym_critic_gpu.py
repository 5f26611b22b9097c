"""The critic window of the fused policy on the GPU (qg_policy_create_asym): proved by BIT EQUALITY with today's code on twin handles, so
no new tolerance enters.  Twin A is FusedMlpPolicy(O, hidden, act, value=False) with the same actor; twin C is FusedMlpPolicy(dim,
hidden, act, value=True) with the same critic, fed the strided view rows[:, off:off + dim].  forward's actions / log_prob are A's and
its value C's; ppo_grad's actor and log_std sections and policy statistics are A's, its critic section and value_loss C's.  Then:
the stride rule, Adam (a fresh handle loaded with params_out continues bit for bit; p, m, v within adam_reference's budget), the
parameter round trip, graph replay, and the window an old-constructor handle reports.
The module's name puts it last in collection, as the other modules that capture hipGraphs on a side stream."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

import adam_reference as AR
import asym_critic_reference as A
import ppo_reference as G

from quadruped_gym_amd import _abi
from quadruped_gym_amd.policy import FusedMlpPolicy, flatten_layers

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
Samples = collections.namedtuple("Samples", G.Batch._fields)
IDS = ["%d-%s-%d-%s" % (s[0], "x".join(map(str, s[1])), s[2], "+".join(map(str, s[3]))) for s in A.SHAPES]


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _nets(shape, seed=0):
    O, hidden, act, window = shape
    return A.make_net(np.random.default_rng(1000 + O + seed), O, hidden, act, window)


def _trio(shape, nets, out_tanh=False, reserve=0):
    """(asymmetric policy, twin A, twin C) holding the same actor, log_std and critic."""
    O, hidden, act, window = shape
    actor, log_std, critic = nets
    asym = FusedMlpPolicy(O, hidden, act, out_tanh=out_tanh, critic_obs=window)
    twin_a = FusedMlpPolicy(O, hidden, act, out_tanh=out_tanh, value=False)
    twin_c = FusedMlpPolicy(window[1], hidden, act, out_tanh=out_tanh, value=True)
    asym.load_layers(actor, log_std, critic)
    twin_a.load_layers(actor, log_std)
    zeros = [(np.zeros(s, np.float32), np.zeros(s[0], np.float32)) for s in twin_c.layer_shapes()[0]]
    twin_c.load_layers(zeros, log_std, critic)
    for p in (asym, twin_a, twin_c):
        if reserve:
            p.reserve_grad(reserve)
    return asym, twin_a, twin_c


def _rows(shape, n, seed, pad=0):
    O, _, _, window = shape
    width = A.row_width(O, window) + pad
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.standard_normal((n, width)) * np.logspace(-2, 1, width)).astype(np.float32)).to(DEV)


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", ["4", "1"])
@pytest.mark.parametrize("shape", A.SHAPES, ids=IDS)
def test_forward_is_the_twins(shape, waves, monkeypatch):
    monkeypatch.setenv("QG_POLICY_WAVES", waves)                # read at create: both launch shapes, whatever the size
    O, hidden, act, (off, dim) = shape
    asym, twin_a, twin_c = _trio(shape, _nets(shape), out_tanh=O == 33)
    assert asym.critic_obs == (off, dim) and asym.asymmetric and asym.n_params == len(flatten_layers(*_nets(shape)))
    for n in (1, 16, 17, 100):
        assert asym.launch_shape(n, value=True)[0] == int(waves) == twin_c.launch_shape(n, value=True)[0]
        rows = _rows(shape, n, seed=n, pad=0 if n != 17 else 3)   # pad 0: the window may end exactly at the stride
        for eps in (None, torch.randn((n, act), device=DEV, generator=torch.Generator(device=DEV).manual_seed(n))):
            out = {k: [torch.full((n, act), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV), torch.full((n,), 7.0, device=DEV)] for k in "sac"}
            asym.forward(rows, out["s"][0], eps=eps, log_prob=out["s"][1], value=out["s"][2])
            twin_a.forward(rows[:, :O], out["a"][0], eps=eps, log_prob=out["a"][1])
            twin_c.forward(rows[:, off:off + dim], out["c"][0], log_prob=out["c"][1], value=out["c"][2])
            torch.cuda.synchronize()
            assert np.array_equal(bits(out["s"][0]), bits(out["a"][0])) and np.array_equal(bits(out["s"][1]), bits(out["a"][1])), n
            assert np.array_equal(bits(out["s"][2]), bits(out["c"][2])), n
            assert out["s"][2].abs().max() > 0 and (out["s"][2] != 7.0).all()
    for p in (asym, twin_a, twin_c):
        p.close()


def test_stride_rule_and_the_old_constructors_window():
    shape = A.SHAPES[2]                                         # O 260, window (260, 85): the critic reads behind the actor's columns
    O, hidden, act, (off, dim) = shape
    asym, twin_a, twin_c = _trio(shape, _nets(shape))
    n = 17
    rows = _rows(shape, n, seed=5)
    narrow = rows[:, :O].contiguous()                           # stride = O
    a1, l1, a2, l2, v = torch.zeros((n, act), device=DEV), torch.zeros(n, device=DEV), torch.zeros((n, act), device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    asym.forward(narrow, a1, log_prob=l1)                       # no value buffer: the critic is not launched, stride O is enough
    twin_a.forward(narrow, a2, log_prob=l2)
    torch.cuda.synchronize()
    assert np.array_equal(bits(a1), bits(a2)) and np.array_equal(bits(l1), bits(l2))
    with pytest.raises(ValueError, match="critic reads columns 260 .. 345"):
        asym.forward(narrow, a1, value=v)
    lib = _abi.load_library()
    assert lib.qg_policy_forward_device(asym._h, n, narrow.data_ptr(), O, None, a1.data_ptr(), None, v.data_ptr(), None) == -1
    assert b"the end of the critic's window" in lib.qg_last_error()
    assert lib.qg_policy_forward_device(asym._h, n, rows.data_ptr(), O + dim - 1, None, a1.data_ptr(), None, v.data_ptr(), None) == -1
    asym.reserve_grad(n)
    grad = torch.zeros(asym.n_params, device=DEV)
    batch = Samples(narrow, a1, l1, l1, l1, l1)
    with pytest.raises(ValueError, match="critic reads columns"):
        asym.ppo_grad(batch, grad)
    assert (grad == 0).all()
    # ONE row has no stride to show what lies behind it: it must be the wide row itself.  A narrow row is refused -- alone in its
    # memory, or with other rows' memory behind it -- and the wide row gives twin C's value
    one, v1, vc = torch.zeros((1, act), device=DEV), torch.full((1,), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
    lone = rows[3, :O].clone().view(1, O)
    for bad in (lone, narrow[:1], narrow[n - 1:]):
        with pytest.raises(ValueError, match="one row of 260 columns"):
            asym.forward(bad, one, value=v1)
        with pytest.raises(ValueError, match="one row of 260 columns"):
            asym.ppo_grad(Samples(bad, one, v1, v1, v1, v1), grad)
    asym.forward(lone, one)                                     # (without the critic the narrow row is all that is read)
    # ... and the last of several rows: 17 rows at the wide stride over memory that ends with the last row's actor columns
    short = rows.reshape(-1)[:(n - 1) * (O + dim) + O].clone().as_strided((n, O), (O + dim, 1))
    with pytest.raises(ValueError, match="memory ends 85 floats"):
        asym.forward(short, a1, value=v)
    torch.cuda.synchronize()
    assert (v1 == 7.0).all() and (v == 0).all() and (grad == 0).all()
    wide_one = rows[3:4].clone()
    twin_c.forward(wide_one[:, off:off + dim], one, value=vc)
    with pytest.raises(ValueError, match="one row of 260 columns"):
        asym.forward(wide_one[:, :O], one, value=v1)            # (its slice shows 260 columns: refused like any narrow row)
    asym.forward(wide_one, one, value=v1)
    torch.cuda.synchronize()
    assert np.array_equal(bits(v1), bits(vc)) and (vc != 7.0).all()
    # handles of the old constructor: the window (0, obs_dim), with or without a critic
    assert twin_a.critic_obs == (0, O) and twin_c.critic_obs == (0, dim) and not twin_a.asymmetric and not twin_c.asymmetric
    off_c, dim_c = C.c_int32(), C.c_int32()
    assert lib.qg_policy_critic_window(twin_c._h, C.byref(off_c), C.byref(dim_c)) == 0 and (off_c.value, dim_c.value) == (0, dim)
    # a window that equals the actor's columns is the symmetric policy, bit for bit
    sym_shape = (33, (64, 64), 12, (0, 33))
    actor, log_std, critic = _nets(sym_shape)
    same, old = FusedMlpPolicy(33, (64, 64), 12, critic_obs=(0, 33)), FusedMlpPolicy(33, (64, 64), 12)
    same.load_layers(actor, log_std, critic), old.load_layers(actor, log_std, critic)
    r33 = _rows(sym_shape, 40, seed=6, pad=2)[:, :33]
    outs = [[torch.zeros((40, 12), device=DEV), torch.zeros(40, device=DEV), torch.zeros(40, device=DEV)] for _ in range(2)]
    same.forward(r33, outs[0][0], log_prob=outs[0][1], value=outs[0][2]), old.forward(r33, outs[1][0], log_prob=outs[1][1], value=outs[1][2])
    torch.cuda.synchronize()
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(*outs)) and np.array_equal(same.params(), old.params())
    assert same.critic_obs == (0, 33) and not same.asymmetric      # SB3's net: load_sb3_state_dict takes it
    for p in (asym, twin_a, twin_c, same, old):
        p.close()


# ---- 2. the PPO gradient ----------------------------------------------------------------------------------------------------------------
def _device_batch(batch, obs):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return Samples(obs, t(batch.actions), t(batch.old_values), t(batch.old_log_prob), t(batch.advantages), t(batch.returns))


def _grad(pol, dbatch, **kw):
    grad, stats = torch.full((pol.n_params,), float("nan"), device=DEV), torch.full((8,), float("nan"), device=DEV)
    pol.ppo_grad(dbatch, grad, stats, ent_coef=0.01, **kw)
    torch.cuda.synchronize()
    return grad, stats


@pytest.mark.parametrize("cv", [None, 0.2])
@pytest.mark.parametrize("shape", A.SHAPES, ids=IDS)
def test_ppo_grad_is_the_twins(shape, cv):
    O, hidden, act, window = shape
    off, dim = window
    nets = _nets(shape, seed=1)
    out_tanh = O == 33
    asym, twin_a, twin_c = _trio(shape, nets, out_tanh=out_tanh, reserve=513)
    lo = asym.param_slices()["critic.0.weight"][0]
    assert lo == twin_a.n_params and asym.n_params - lo == twin_c.n_params - twin_c.param_slices()["critic.0.weight"][0]
    for B in (1, 17, 513):
        rng = np.random.default_rng(B)
        batch = A.make_batch(rng, *nets, O, window, out_tanh, B, clip_range_vf=cv)
        rows = torch.from_numpy(batch.observations).to(DEV)
        assert rows.shape[1] == A.row_width(O, window)
        g_s, s_s = _grad(asym, _device_batch(batch, rows), clip_range_vf=cv)
        g_a, s_a = _grad(twin_a, _device_batch(batch._replace(old_values=None, returns=None), rows[:, :O]))
        g_c, s_c = _grad(twin_c, _device_batch(batch, rows[:, off:off + dim]), clip_range_vf=cv)
        assert np.array_equal(bits(g_s[:lo]), bits(g_a)), B                               # actor and log_std sections
        assert np.array_equal(bits(g_s[lo:]), bits(g_c[twin_c.n_params - (asym.n_params - lo):])), B      # the critic section
        assert np.array_equal(bits(s_s[[1, 4, 5]]), bits(s_a[[1, 4, 5]])) and np.array_equal(bits(s_s[2:3]), bits(s_c[2:3])), B
        assert torch.isfinite(g_s).all() and g_s[lo:].abs().max() > 0 and s_s[2] > 0
        if B == 513 and cv is None:                            # and the bits are a gradient: against the float64 composition
            _, want = A.loss_and_grad(*nets, batch, O, window, out_tanh, 0.2, cv, 0.01, 0.5)
            err = np.abs(g_s.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max()
            print("%s B %d: largest |gpu - f64| / largest |f64| = %.2e" % (shape, B, err))
            assert err < 1e-5                                   # (the pass keeps f32 activations: ~1e-7 a term; test_ppo_gpu.py holds the symmetric pass tighter)
    for p in (asym, twin_a, twin_c):
        p.close()


# ---- 3. Adam, the round trip, graph replay --------------------------------------------------------------------------------------------------
def test_adam_step_round_trip_and_graph_replay():
    shape = A.SHAPES[1]                                         # (33, (64, 64), 12, (0, 118))
    O, hidden, act, window = shape
    nets = _nets(shape, seed=2)
    B = 100
    batch = A.make_batch(np.random.default_rng(9), *nets, O, window, False, B, clip_range_vf=0.2)
    rows = torch.from_numpy(batch.observations).to(DEV)
    dbatch = _device_batch(batch, rows)

    def fresh(params=None):
        p = FusedMlpPolicy(O, hidden, act, critic_obs=window)
        p.load_layers(*nets) if params is None else p.set_params(params)
        p.reserve_grad(B), p.reserve_adam()
        return p

    def outputs(p):
        a, l, v = torch.zeros((B, act), device=DEV), torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
        p.forward(rows, a, log_prob=l, value=v)
        g, s = _grad(p, dbatch, clip_range_vf=0.2)
        return [bits(x) for x in (a, l, v, g, s)]

    pol = fresh()
    p0 = pol.params()
    assert np.array_equal(p0, flatten_layers(*nets))            # set / get round trip, asymmetric layout
    t = torch.from_numpy(p0[::-1].copy()).to(DEV)
    pol.update_from(t)
    assert np.array_equal(pol.params(), p0[::-1])
    pol.update_from(torch.from_numpy(p0).to(DEV))
    eager0 = outputs(pol)
    grad, _ = _grad(pol, dbatch, clip_range_vf=0.2)
    params_out = torch.zeros(pol.n_params, device=DEV)
    # (adam_reference's constants are float32 values: what the launch receives is what the float64 restatement uses)
    pol.adam_step(grad, lr=AR.LR, betas=(AR.BETA1, AR.BETA2), eps=AR.EPS, max_grad_norm=AR.MAX_NORM, params_out=params_out)
    torch.cuda.synchronize()
    after = outputs(pol)
    new = params_out.cpu().numpy()
    assert np.array_equal(new, pol.params()) and not np.array_equal(new, p0)
    other = fresh(new)                                          # a fresh asymmetric handle loaded with params_out: the same bits
    assert all(np.array_equal(x, y) for x, y in zip(after, outputs(other)))
    # p, m, v against float64 within adam_reference's budget
    g64 = grad.cpu().numpy().astype(np.float64)
    z = np.zeros_like(g64)
    p64, m64, v64, _, _ = AR.clip_and_adam(p0.astype(np.float64), z, z, 0, g64, AR.LR, AR.BETA1, AR.BETA2, AR.EPS, AR.MAX_NORM, np.float64)
    tol_p, tol_m, tol_v = AR.gpu_tolerances(p64, m64, v64, lr=AR.LR)
    state = pol.adam_state()
    assert state["step"] == 1
    assert (np.abs(new - p64) <= tol_p).all() and (np.abs(state["exp_avg"] - m64) <= tol_m).all() and (np.abs(state["exp_avg_sq"] - v64) <= tol_v).all()
    # graph replay of forward + ppo_grad equals the eager run
    cap = fresh()
    a, l, v = torch.zeros((B, act), device=DEV), torch.zeros(B, device=DEV), torch.zeros(B, device=DEV)
    g, s = torch.zeros(cap.n_params, device=DEV), torch.zeros(8, device=DEV)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap.forward(rows, a, log_prob=l, value=v, stream=side)
        cap.ppo_grad(dbatch, g, s, ent_coef=0.01, clip_range_vf=0.2, stream=side)
    for x in (a, l, v, g, s):
        x.zero_()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert all(np.array_equal(x, bits(y)) for x, y in zip(eager0, (a, l, v, g, s)))
    del graph
    for p in (pol, other, cap):
        p.close()
