"""The fused MLP policy on the GPU (qg_policy_*, csrc/qg_policy.hip) against the float64 checker of tests/policy_reference.py.

Tolerance of the forward pass (case 1, also the log-probability of case 5): no fixed figure.  Each case computes the error of the torch
float32 policy ON THE GPU -- the path the kernel replaces -- against the float64 checker on the same inputs; the fused kernel's maximum
absolute error may be at most 4x that (a sequential k-ordered sum against the library's blocked one, and another tanh), with a floor
of 1e-6 absolute.
With QG_POLICY_PARITY_OUT=<file> every case appends both paths' maxima to that file (profiles/r08/policy_parity.txt)."""
import math
import zlib

import numpy as np
import pytest
import torch

import policy_reference as R
from policy_checks import DEV, bound, observations, record, run, torch_tower

from quadruped_gym_amd import _abi
from quadruped_gym_amd.policy import FusedMlpPolicy

pytestmark = pytest.mark.gpu


def _make(shape, out_tanh, value, init, seed, log_std=None):
    obs_dim, hidden, act_dim = R.SHAPES[shape]
    rng = np.random.default_rng(seed)
    actor = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, act_dim), init)
    critic = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, 1), init, head_gain=1.0) if value else None
    if log_std is None:
        log_std = rng.uniform(-1.5, 0.3, act_dim).astype(np.float32)
    pol = FusedMlpPolicy(obs_dim, hidden, act_dim, out_tanh=out_tanh, value=value)
    pol.load_layers(actor, log_std, critic)
    return pol, actor, critic, log_std, rng


# ---- 1. forward against the float64 checker ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 17, 4096, 5000])
@pytest.mark.parametrize("value", [False, True])
@pytest.mark.parametrize("out_tanh", [False, True])
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_forward_matches_float64_checker(shape, out_tanh, value, n):
    obs_dim = R.SHAPES[shape][0]
    for init in ("sb3", "linear"):
        pol, actor, critic, log_std, rng = _make(shape, out_tanh, value, init, seed=zlib.crc32(repr((shape, out_tanh, value, n, init)).encode()))
        obs = observations(rng, n, obs_dim)
        eps = rng.standard_normal((n, pol.act_dim)).astype(np.float32)
        mean_ref, act_ref, lp_ref, val_ref = R.forward(actor, log_std, obs, eps=eps, critic=critic, out_tanh=out_tanh)

        # the path being replaced: torch float32 on the GPU
        with torch.no_grad():
            x = torch.from_numpy(obs).to(DEV)
            t_mean = torch_tower(actor, out_tanh)(x)
            std = torch.from_numpy(log_std).to(DEV).exp()
            t_act = t_mean + std * torch.from_numpy(eps).to(DEV)
            t_lp = torch.distributions.Normal(t_mean, std).log_prob(t_act).sum(-1)
            t_val = torch_tower(critic, False)(x)[:, 0] if value else None
        terr = {"mean": np.abs(t_mean.cpu().numpy() - mean_ref).max(), "log_prob": np.abs(t_lp.cpu().numpy() - lp_ref).max()}
        if value:
            terr["value"] = np.abs(t_val.cpu().numpy() - val_ref).max()

        # observations contiguous, and in place out of a wider row buffer whose other columns hold a sentinel
        wide = torch.full((n, obs_dim + 2), 1.0e30, device=DEV)
        wide[:, :obs_dim] = torch.from_numpy(obs).to(DEV)
        outs = {}
        for layout, obs_t in (("contiguous", torch.from_numpy(obs).to(DEV)), (f"stride {obs_dim + 2}", wide[:, :obs_dim])):
            mean, _, val = run(pol, obs_t, None, want_lp=False)
            act, lp, _ = run(pol, obs_t, torch.from_numpy(eps).to(DEV))
            outs[layout] = (mean, act, lp, val)
            ferr = {"mean": np.abs(mean - mean_ref).max(), "log_prob": np.abs(lp - lp_ref).max()}
            if value:
                ferr["value"] = np.abs(val - val_ref).max()
            refs = {"mean": mean_ref, "log_prob": lp_ref, "value": val_ref}
            record(f"{shape} out_tanh={int(out_tanh)} critic={int(value)} n={n} init={init} obs={layout}: " +
                    "  ".join(f"{k}: fused {ferr[k]:.3e} torch {terr[k]:.3e} bound {bound(terr[k], refs[k]):.3e}" for k in ferr))
            for k in ferr:
                assert np.isfinite(ferr[k]) and ferr[k] <= bound(terr[k], refs[k]), (k, layout, init, ferr[k], terr[k])
        a, b = outs["contiguous"], outs[f"stride {obs_dim + 2}"]
        assert all(np.array_equal(u, v) for u, v in zip(a, b) if u is not None)      # the row stride changes nothing
        pol.close()


# ---- 2. exact-integer layout check ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 20000])           # four waves per env tile, and one
@pytest.mark.parametrize("hidden", [64, 256])
def test_layout_with_exact_integers(hidden, n):
    """Integer observations and an integer, asymmetric first-layer matrix scaled by 2^-16 keep every hidden pre-activation z = I x 2^-16
    exact and inside +-2^-6 (|I| <= 33 x 12 + 8 < 1024), where tanh(z) = z (1 - z^2 / 3 ..): I tanh(z) / z is within 2^-13 |I| < 0.13 of
    the integer I.  The second layer is a selector (2^16 at one hidden unit per action, bias = the action's index), so every output is
    within 0.2 of the integer I[unit] + index: a transposed or k-permuted fragment anywhere gives another integer, not a small error."""
    obs_dim, act_dim = 33, 16
    rng = np.random.default_rng(7)
    W1 = rng.integers(-3, 4, (hidden, obs_dim)).astype(np.float64)
    W1[:, 0] = np.arange(hidden) % 7 - 3               # rows and columns are all distinguishable
    b1 = rng.integers(-8, 9, hidden).astype(np.float64)
    obs = rng.integers(-4, 5, (n, obs_dim)).astype(np.float32)
    I = obs.astype(np.float64) @ W1.T + b1
    assert np.abs(I).max() < 1024
    pol = FusedMlpPolicy(obs_dim, (hidden,), act_dim, out_tanh=False, value=False)
    obs_t = torch.from_numpy(obs).to(DEV)
    perm = rng.permutation(hidden)                      # which hidden unit each action of each round selects
    for r in range(hidden // act_dim):
        units = perm[r * act_dim:(r + 1) * act_dim]
        W2 = np.zeros((act_dim, hidden))
        W2[np.arange(act_dim), units] = 2.0 ** 16
        pol.load_layers([(W1 * 2.0 ** -16, b1 * 2.0 ** -16), (W2, np.arange(act_dim, dtype=np.float64))], np.zeros(act_dim))
        act, _, _ = run(pol, obs_t, None, want_lp=False)
        want = I[:, units] + np.arange(act_dim)
        assert np.abs(act - want).max() < 0.2, (r, np.abs(act - want).max())
        assert np.array_equal(np.rint(act), want)
    pol.close()


# ---- 3. row independence, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_rows_are_independent_bit_for_bit(shape):
    pol, _, _, _, rng = _make(shape, True, True, "sb3", seed=11)
    obs_dim = R.SHAPES[shape][0]
    obs = observations(rng, 4096, obs_dim)
    eps = rng.standard_normal((4096, pol.act_dim)).astype(np.float32)
    big = run(pol, torch.from_numpy(obs).to(DEV), torch.from_numpy(eps).to(DEV))
    for i in (0, 5, 1234, 4095):
        one = run(pol, torch.from_numpy(obs[i:i + 1]).to(DEV), torch.from_numpy(eps[i:i + 1]).to(DEV))
        for u, v in zip(big, one):
            assert np.array_equal(u[i:i + 1], v)
        # the same row at the end of other batches: a masked tail tile (5000), and the one-wave-per-tile launch (20000)
        for m in (5000, 20000):
            o2, e2 = observations(rng, m, obs_dim), rng.standard_normal((m, pol.act_dim)).astype(np.float32)
            o2[m - 1], e2[m - 1] = obs[i], eps[i]
            other = run(pol, torch.from_numpy(o2).to(DEV), torch.from_numpy(e2).to(DEV))
            for u, v in zip(big, other):
                assert np.array_equal(u[i], v[m - 1])
    pol.close()


# ---- 4. parameter round trip and the stream-ordered update --------------------------------------------------------------------------
def test_param_round_trip_and_device_update():
    pol, actor, critic, log_std, rng = _make("po", False, True, "linear", seed=5)
    flat = R.flatten(actor, log_std, critic)
    assert flat.shape == (pol.n_params,) and np.array_equal(pol.params(), flat)
    with pytest.raises(ValueError):
        pol.set_params(flat[:-1])

    n = 300
    obs = torch.from_numpy(observations(rng, n, pol.obs_dim)).to(DEV)
    actor2 = R.random_layers(rng, R.tower_shapes(260, (64, 64), 12), "sb3", head_gain=1.0)
    critic2 = R.random_layers(rng, R.tower_shapes(260, (64, 64), 1), "sb3", head_gain=1.0)
    flat2 = R.flatten(actor2, log_std, critic2)
    new = torch.from_numpy(flat2).to(DEV)
    a_old, a_new = torch.empty((n, 12), device=DEV), torch.empty((n, 12), device=DEV)
    v_old, v_new = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):                      # old forward, update, new forward: ordered by the stream alone
        pol.forward(obs, a_old, value=v_old)
        pol.update_from(new)
        pol.forward(obs, a_new, value=v_new)
    side.synchronize()
    assert np.array_equal(pol.params(), flat2)
    ref_old = R.forward(actor, log_std, obs.cpu().numpy(), critic=critic)
    ref_new = R.forward(actor2, log_std, obs.cpu().numpy(), critic=critic2)
    assert np.abs(a_old.cpu().numpy() - ref_old[0]).max() < 1e-5 and np.abs(v_old.cpu().numpy() - ref_old[3]).max() < 1e-5
    assert np.abs(a_new.cpu().numpy() - ref_new[0]).max() < 1e-5 and np.abs(v_new.cpu().numpy() - ref_new[3]).max() < 1e-5
    assert np.abs(ref_new[0] - ref_old[0]).max() > 1e-2           # the two parameter sets are told apart
    # the same parameters through the host path give the same bits
    twin = FusedMlpPolicy(260, (64, 64), 12, out_tanh=False, value=True)
    twin.set_params(flat2)
    a_twin = torch.empty((n, 12), device=DEV)
    twin.forward(obs, a_twin)
    torch.cuda.synchronize()
    assert torch.equal(a_twin, a_new)
    twin.close()
    pol.close()


def test_forward_refuses_bad_tensors():
    pol = FusedMlpPolicy(33, (64, 64), 12, value=False)
    obs, act = torch.zeros((8, 33), device=DEV), torch.zeros((8, 12), device=DEV)
    with pytest.raises(ValueError):
        pol.forward(obs, act, value=torch.zeros(8, device=DEV))          # no critic tower
    with pytest.raises(ValueError):
        pol.forward(obs.double(), act)                                    # dtype
    with pytest.raises(ValueError):
        pol.forward(torch.zeros((33, 8), device=DEV).t(), act)          # rows not contiguous
    with pytest.raises(ValueError):
        pol.forward(obs, torch.zeros((8, 16), device=DEV)[:, :12])      # actions must be contiguous
    with pytest.raises(ValueError):
        pol.forward(obs.cpu(), act)
    lib = _abi.load_library()
    assert lib.qg_policy_forward_device(pol._h, 8, obs.data_ptr(), 32, None, act.data_ptr(), None, None, None) == -1     # stride < obs_dim
    assert lib.qg_policy_forward_device(pol._h, 0, obs.data_ptr(), 33, None, act.data_ptr(), None, None, None) == -1
    assert lib.qg_policy_forward_device(pol._h, 8, obs.data_ptr(), 33, None, act.data_ptr(), None, act.data_ptr(), None) == -1   # value, no critic
    pol.close()


# ---- 5. sampling ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["plain", "po_wide"])
def test_sampling_and_log_prob(shape):
    pol, actor, critic, log_std, rng = _make(shape, False, True, "sb3", seed=21)
    n = 5000
    obs = observations(rng, n, pol.obs_dim)
    eps = rng.standard_normal((n, pol.act_dim)).astype(np.float32)
    obs_t, eps_t = torch.from_numpy(obs).to(DEV), torch.from_numpy(eps).to(DEV)
    mean, lp0, _ = run(pol, obs_t, None)
    act, lp, _ = run(pol, obs_t, eps_t)
    # the action from the kernel's own mean, in float32 as the formula reads; std = exp(log_std) correctly rounded
    std = np.exp(log_std.astype(np.float64)).astype(np.float32)
    want = mean + std * eps
    assert np.abs(act - want).max() <= np.spacing(np.abs(want)).max() and np.all(np.abs(act - want) <= np.spacing(np.abs(want)))
    # log-probability: the tolerance rule of case 1
    _, _, lp_ref, _ = R.forward(actor, log_std, obs, eps=eps)
    with torch.no_grad():
        t_mean = torch_tower(actor, False)(obs_t)
        t_std = torch.from_numpy(log_std).to(DEV).exp()
        t_lp = torch.distributions.Normal(t_mean, t_std).log_prob(t_mean + t_std * eps_t).sum(-1).cpu().numpy()
    terr, ferr = np.abs(t_lp - lp_ref).max(), np.abs(lp - lp_ref).max()
    record(f"{shape} sampling n={n}: log_prob: fused {ferr:.3e} torch {terr:.3e} bound {bound(terr, lp_ref):.3e}")
    assert ferr <= bound(terr, lp_ref)
    # no eps: the log-density at the mean, the same for every row
    at_mean = float((-log_std.astype(np.float64) - 0.5 * math.log(2 * math.pi)).sum())
    assert np.all(lp0 == lp0[0]) and abs(float(lp0[0]) - at_mean) <= np.spacing(np.float32(abs(at_mean)))
    pol.close()


# ---- 6. hipGraph replays the eager bits -----------------------------------------------------------------------------------------------
def _auto_reset_task():
    t = _abi.default_task()
    t.auto_reset, t.use_fall, t.fall_height = 1, 1, 0.05
    return t


def test_graph_replays_eager_bits_plain_step():
    from quadruped_gym_amd.sim import BatchedSim
    n, G = 4096, 8
    pol, _, _, _, rng = _make("plain", True, True, "linear", seed=31)
    sim = BatchedSim(n, task=_auto_reset_task())
    sim.reset(seed=3)
    snap = sim.snapshot()
    rows, acts = torch.zeros((n, 35), device=DEV), torch.zeros((n, 12), device=DEV)
    lp, val = torch.zeros((G, n), device=DEV), torch.zeros((G, n), device=DEV)
    eps = torch.randn((G, n, 12), device=DEV)

    def loop():
        for k in range(G):
            pol.forward(rows[:, :33], acts, eps=eps[k], log_prob=lp[k], value=val[k])       # reads the packed rows in place
            sim.step_device_packed(acts, rows)

    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        loop()
    side.synchronize()
    eager = [t.clone() for t in (rows, acts, lp, val)]
    sim.restore(snap)
    for t in (rows, acts, lp, val):
        t.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        loop()
    with torch.cuda.stream(side):
        graph.replay()
    side.synchronize()
    torch.cuda.synchronize()
    for a, b in zip(eager, (rows, acts, lp, val)):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    assert float(rows[:, :33].abs().max()) > 0
    sim.close()
    pol.close()


def test_graph_replays_eager_bits_po_step():
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
    n, G = 4096, 8
    env = POWalkingQuadrupedVecEnv(n, obs_window=10, random_controls=True, random_init=True, device_commands=True,
                                   reset_options={"min_speed": 0.0, "max_speed": 0.5}, settling_time=0.5, max_time=10.0)
    assert env.obs_dim == 260
    pol, _, _, _, rng = _make("po", True, True, "linear", seed=32)
    obs0 = torch.from_numpy(env.reset()).to(DEV)
    snap = env.snapshot()
    obs = obs0.clone()
    rew, done = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV, dtype=torch.uint8)
    acts = torch.zeros((n, 12), device=DEV)
    val = torch.zeros((G, n), device=DEV)

    def loop():
        for k in range(G):
            pol.forward(obs, acts, value=val[k])
            env.step_tensor(acts, obs, rew, done)

    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        loop()
    side.synchronize()
    eager = [t.clone() for t in (obs, acts, val, rew.nan_to_num(), done)]
    env.restore(snap)
    obs.copy_(obs0)
    for t in (acts, val, rew, done):
        t.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        loop()
    with torch.cuda.stream(side):
        graph.replay()
    side.synchronize()
    torch.cuda.synchronize()
    for a, b in zip(eager, (obs, acts, val, rew.nan_to_num(), done)):
        assert torch.equal(a, b)
    assert torch.isfinite(obs).all() and torch.isfinite(acts).all() and torch.isfinite(val).all()
    env.close()
    pol.close()


# ---- 7. the closed loop is finite and alive -------------------------------------------------------------------------------------------
def test_closed_loop_is_finite_and_alive():
    from quadruped_gym_amd.sim import BatchedSim
    n, steps = 4096, 200
    pol, _, _, _, rng = _make("plain", True, True, "linear", seed=41, log_std=np.full(12, -0.5, np.float32))
    task = _auto_reset_task()
    task.max_time = 1.0                                 # 125 env-steps: every robot that does not fall first runs into the time limit
    sim = BatchedSim(n, task=task)
    sim.reset(seed=1)
    rows, acts = torch.zeros((n, 35), device=DEV), torch.zeros((n, 12), device=DEV)
    lp, val = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    eps = torch.randn((steps, n, 12), device=DEV)
    ended = torch.zeros(n, device=DEV)
    finite = torch.ones((), device=DEV, dtype=torch.bool)
    for k in range(steps):
        pol.forward(rows[:, :33], acts, eps=eps[k], log_prob=lp, value=val)
        sim.step_device_packed(acts, rows)
        ended += rows[:, 34]
        finite &= torch.isfinite(rows).all() & torch.isfinite(acts).all() & torch.isfinite(lp).all() & torch.isfinite(val).all()
        if k == 49:
            torch.cuda.synchronize()
            assert sim.get_state()[4].max() == 50 * task.frame_skip     # nstep advances: 50 env-steps of frame_skip substeps
    torch.cuda.synchronize()
    assert bool(finite)
    assert int(ended.sum()) >= n                        # every robot's episode ended at least once (and was reset inside the step)
    nstep = sim.get_state()[4]
    assert 0 < nstep.max() <= sim.limit_substeps        # ... and started over
    assert float(acts.abs().max()) > 0 and float(rows[:, :33].abs().max()) > 0
    sim.close()
    pol.close()
