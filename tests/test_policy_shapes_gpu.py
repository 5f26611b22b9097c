"""The fused MLP policy over the shapes its ABI accepts: every row of tests/policy_reference.py's SHAPE_TABLE at one and at four waves
per env tile, so that each of the four instantiations of qg_policy_forward_kernel meets every branch condition it can meet (the census
of tests/test_policy_api.py says which).  Every case first asserts the launch shape the library reports against the host-side rule
(policy_reference.launch_shape): a case that set QG_POLICY_WAVES and got another kernel would fail, not pass on the default one.

No physics: n = 83 rows (five full tiles and a three-row tail), 1 and 17 for the bit checks.

Tolerance of (a) -- the rule of tests/test_policy_gpu.py, measured per case against the path the kernel replaces (torch float32 modules
on the same GPU and inputs, both against the float64 checker): fused <= max(FACTOR x torch, floor), floor = max(1e-6, 4 x the float32
spacing at the largest reference magnitude of that output) -- an f32 result cannot be asked for less than a few ulp of its own size
(value heads here reach |v| = 2.7, where an ulp is 2.4e-7).  FACTOR is the project's 4: measured on an MI355X over the whole table the
worst ratio of a fused error to its bound is 0.50 (value, 33-144-12; action mean 0.33, log-probability 0.12).
With QG_POLICY_PARITY_OUT=<file> every case of (a) appends its maxima and bounds to that file (profiles/r11/policy_shape_parity.txt)."""
import functools
import zlib

import numpy as np
import pytest
import torch

import parity
import policy_reference as R
from policy_checks import DEV, observations, record, run, torch_tower

from quadruped_gym_amd.policy import FusedMlpPolicy

pytestmark = pytest.mark.gpu
N = 83
FACTOR = 4.0
INITS = ("sb3", "linear")
TABLE = range(len(R.SHAPE_TABLE))
_FIRST_WIDE = next(i for i in TABLE if max(R.SHAPE_TABLE[i][1]) > 64)
# out_tanh alternates along the table; the first two narrow and the first two wide rows run both
TANH_CASES = sorted({(i, bool(i % 2)) for i in TABLE} | {(i, t) for i in (0, 1, _FIRST_WIDE, _FIRST_WIDE + 1) for t in (False, True)})


def _id(i):
    obs_dim, hidden, act_dim = R.SHAPE_TABLE[i]
    return "%d-%s-%d" % (obs_dim, "-".join(str(h) for h in hidden), act_dim)


@functools.lru_cache(maxsize=None)
def _inputs(i, init):
    """Parameters and inputs of table row i, made once and read-only: actor, critic, log_std ~ U(-1.5, 0.3), observations with
    per-column scales 0.01 .. 10, eps."""
    obs_dim, hidden, act_dim = R.SHAPE_TABLE[i]
    rng = np.random.default_rng(zlib.crc32(repr((R.SHAPE_TABLE[i], init)).encode()))
    actor = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, act_dim), init)
    critic = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, 1), init, head_gain=1.0)
    log_std = rng.uniform(-1.5, 0.3, act_dim).astype(np.float32)
    obs = observations(rng, N, obs_dim)
    eps = rng.standard_normal((N, act_dim)).astype(np.float32)
    for a in [log_std, obs, eps] + [x for W, b in actor + critic for x in (W, b)]:
        a.setflags(write=False)
    return actor, critic, log_std, obs, eps


@functools.lru_cache(maxsize=None)
def _reference(i, init, out_tanh):
    """The float64 checker on row i's inputs: (mean, log_prob, value), read-only."""
    actor, critic, log_std, obs, eps = _inputs(i, init)
    mean, _, lp, val = R.forward(actor, log_std, obs, eps=eps, critic=critic, out_tanh=out_tanh)
    for a in (mean, lp, val):
        a.setflags(write=False)
    return mean, lp, val


def _make(i, init, out_tanh, waves, monkeypatch):
    """A policy of table row i with QG_POLICY_WAVES pinned (0: unset), and a check that it launches what the rule says."""
    obs_dim, hidden, act_dim = R.SHAPE_TABLE[i]
    if waves:
        monkeypatch.setenv("QG_POLICY_WAVES", str(waves))
    else:
        monkeypatch.delenv("QG_POLICY_WAVES", raising=False)
    actor, critic, log_std, _, _ = _inputs(i, init)
    pol = FusedMlpPolicy(obs_dim, hidden, act_dim, out_tanh=out_tanh, value=True)
    pol.load_layers(actor, log_std, critic)
    for n in (1, 17, N):
        for value in (False, True):
            want = R.launch_shape(hidden, n, 2 if value else 1, parity.simds(), force_waves=waves)
            assert pol.launch_shape(n, value) == want, (n, value, pol.launch_shape(n, value), want)
            assert not waves or want[0] == waves
    return pol


def _t(a):
    return torch.tensor(a, device=DEV)               # a copy: the cached inputs are read-only


def _sampled(pol, obs, eps):
    """(action, log_prob, value) of a sampled forward pass; outputs pre-filled with NaN by run."""
    return run(pol, obs if torch.is_tensor(obs) else _t(obs), _t(eps))


def _same_bits(a, b, rows=slice(None)):
    return all(np.array_equal(u[rows], v[rows]) for u, v in zip(a, b))


def _bound(torch_err, ref):
    return max(FACTOR * torch_err, 1e-6, 4.0 * float(np.spacing(np.float32(np.abs(ref).max()))))


# ---- the default choice ------------------------------------------------------------------------------------------------------------
def test_default_launch_shape_follows_the_rule(monkeypatch):
    """Without QG_POLICY_WAVES: four waves for the wide rows at both sizes; the narrow ones change to one wave where tiles x towers
    reaches the SIMD count (n = 16 x SIMDs: one tile per SIMD with the actor alone)."""
    monkeypatch.delenv("QG_POLICY_WAVES", raising=False)
    simds = parity.simds()
    seen = set()
    for i in TABLE:
        obs_dim, hidden, act_dim = R.SHAPE_TABLE[i]
        pol = FusedMlpPolicy(obs_dim, hidden, act_dim, value=True)
        for n in (N, 16 * simds):
            for value in (False, True):
                got = pol.launch_shape(n, value)
                assert got == R.launch_shape(hidden, n, 2 if value else 1, simds, force_waves=0), (_id(i), n, value, got)
                seen.add(got)
        pol.close()
    assert seen == {(4, 1), (4, 4), (1, 4)}            # <1,16> is reached by QG_POLICY_WAVES=1 alone: every case below runs it


# ---- a. forward against the float64 checker ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("i,out_tanh", TANH_CASES, ids=["%s-tanh%d" % (_id(i), t) for i, t in TANH_CASES])
def test_forward_matches_float64_checker(i, out_tanh, waves, monkeypatch):
    for init in INITS:
        actor, critic, log_std, obs, eps = _inputs(i, init)
        refs = dict(zip(("mean", "log_prob", "value"), _reference(i, init, out_tanh)))
        pol = _make(i, init, out_tanh, waves, monkeypatch)
        with torch.no_grad():                          # the path being replaced: torch float32 on the GPU
            x = _t(obs)
            t_mean = torch_tower(actor, out_tanh)(x)
            std = _t(log_std).exp()
            t_act = t_mean + std * _t(eps)
            t_lp = torch.distributions.Normal(t_mean, std).log_prob(t_act).sum(-1)
            t_val = torch_tower(critic, False)(x)[:, 0]
        terr = {"mean": np.abs(t_mean.cpu().numpy() - refs["mean"]).max(), "log_prob": np.abs(t_lp.cpu().numpy() - refs["log_prob"]).max(),
                "value": np.abs(t_val.cpu().numpy() - refs["value"]).max()}
        mean, _, val = run(pol, x, None, want_lp=False)
        _, lp, val2 = _sampled(pol, x, eps)
        assert np.array_equal(val, val2)
        ferr = {"mean": np.abs(mean - refs["mean"]).max(), "log_prob": np.abs(lp - refs["log_prob"]).max(),
                "value": np.abs(val - refs["value"]).max()}
        bound = {k: _bound(terr[k], refs[k]) for k in ferr}
        record(f"{_id(i)} out_tanh={int(out_tanh)} waves={waves} blocks={pol.launch_shape(N, True)[1]} init={init}: " +
                "  ".join(f"{k}: fused {ferr[k]:.3e} torch {terr[k]:.3e} bound {bound[k]:.3e} ratio {ferr[k] / bound[k]:.2f}" for k in ferr))
        for k in ferr:
            assert np.isfinite(ferr[k]) and ferr[k] <= bound[k], (k, init, ferr[k], terr[k], bound[k])
        pol.close()


# ---- b. the launch shape changes no bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", TABLE, ids=_id)
def test_launch_shape_changes_no_bit(i, monkeypatch):
    for init in INITS:
        _, _, _, obs, eps = _inputs(i, init)
        outs = {}
        for waves in (1, 4):
            pol = _make(i, init, bool(i % 2), waves, monkeypatch)
            outs[waves] = _sampled(pol, obs, eps)
            pol.close()
        assert all(np.isfinite(u).all() for u in outs[1])
        assert _same_bits(outs[1], outs[4]), init


# ---- c. rows are independent in every instantiation --------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("i", TABLE, ids=_id)
def test_rows_are_independent_bit_for_bit(i, waves, monkeypatch):
    for init in INITS:
        _, _, _, obs, eps = _inputs(i, init)
        pol = _make(i, init, bool(i % 2), waves, monkeypatch)
        big = _sampled(pol, obs, eps)
        assert all(np.isfinite(u).all() for u in big)
        for n in (1, 17):
            part = _sampled(pol, obs[:n], eps[:n])         # a row the kernel does not write stays NaN and fails the comparison
            assert all(u.shape[0] == n for u in part) and _same_bits(part, [u[:n] for u in big]), n
        pol.close()


# ---- d. a bad row stays in its row -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("i", TABLE, ids=_id)
def test_a_bad_row_stays_in_its_row(i, waves, monkeypatch):
    """Row 20 all NaN, row 37 with +inf in column 0, row 82 all NaN -- the last live row of the tail tile, which the clamped loads of
    the dead rows read.  The bad rows' own outputs are unspecified and not looked at."""
    for init in INITS:
        _, _, _, obs, eps = _inputs(i, init)
        pol = _make(i, init, bool(i % 2), waves, monkeypatch)
        clean = _sampled(pol, obs, eps)
        bad = obs.copy()
        bad[20], bad[37, 0], bad[82] = np.nan, np.inf, np.nan
        dirty = _sampled(pol, bad, eps)
        good = np.ones(N, bool)
        good[[20, 37, 82]] = False
        assert all(np.isfinite(u[good]).all() for u in dirty)
        assert _same_bits(clean, dirty, good)
        pol.close()


# ---- e. row stride -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("i", [i for i in TABLE if R.SHAPE_TABLE[i][0] in (1, 17, 260, 512)], ids=_id)
def test_odd_row_stride_changes_no_bit(i, waves, monkeypatch):
    """Observations read in place out of a buffer one float wider (an odd stride for the even widths, 2 for obs_dim 1), the spare
    column holding 1e30."""
    obs_dim = R.SHAPE_TABLE[i][0]
    for init in INITS:
        _, _, _, obs, eps = _inputs(i, init)
        pol = _make(i, init, bool(i % 2), waves, monkeypatch)
        wide = torch.full((N, obs_dim + 1), 1.0e30, device=DEV)
        wide[:, :obs_dim] = _t(obs)
        view = wide[:, :obs_dim]
        assert view.stride() == (obs_dim + 1, 1)
        contiguous, strided = _sampled(pol, obs, eps), _sampled(pol, view, eps)
        assert all(np.isfinite(u).all() for u in contiguous) and _same_bits(contiguous, strided)
        pol.close()


# ---- f. exact-integer layout check in a second position ----------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("obs_dim,hidden", [(16, 48), (64, 208)])
def test_layout_with_exact_integers(obs_dim, hidden, waves, monkeypatch):
    """The construction of tests/test_policy_gpu.py's test of this name (integer observations in -4 .. 4, an integer first-layer matrix
    in -3 .. 3 scaled by 2^-16, a selector second layer: every output within 0.2 of a known integer, and a transposed or k-permuted
    fragment gives another integer) where the first layer has no padding (16 and 64 inputs) and where the four waves hold different
    block counts (208 wide: 4/3/3/3).  |I| <= 64 x 12 + 8 < 1024 keeps z = I x 2^-16 inside +-2^-6 as there."""
    act_dim = 16
    monkeypatch.setenv("QG_POLICY_WAVES", str(waves))
    rng = np.random.default_rng(7)
    W1 = rng.integers(-3, 4, (hidden, obs_dim)).astype(np.float64)
    W1[:, 0] = np.arange(hidden) % 7 - 3               # rows and columns are all distinguishable
    b1 = rng.integers(-8, 9, hidden).astype(np.float64)
    obs = rng.integers(-4, 5, (N, obs_dim)).astype(np.float32)
    I = obs.astype(np.float64) @ W1.T + b1
    assert np.abs(I).max() < 1024
    pol = FusedMlpPolicy(obs_dim, (hidden,), act_dim, out_tanh=False, value=False)
    assert pol.launch_shape(N) == R.launch_shape((hidden,), N, 1, parity.simds(), force_waves=waves)
    obs_t = _t(obs)
    perm = rng.permutation(hidden)                      # which hidden unit each action of each round selects
    assert hidden % act_dim == 0
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
