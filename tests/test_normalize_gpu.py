"""The running normaliser on the GPU (qg_norm_*, csrc/qg_norm.hip) against the float64 checker of tests/normalize_reference.py.

Statistics after six training steps: |d mean| <= 1e-12 max|x| and |d var| <= 1e-9 var + (1e-12 max|x|)^2 per column, max|x| over
everything the column has seen; the count exactly; the returns and their statistic within 1e-12 of the largest |return|.  Outputs:
within one float32 ulp of the step 2 / step 4 formula evaluated in float64 with the statistics the device itself reports, clipped
elements exactly at the clip.  Everything else here is bit-for-bit identity.
With QG_NORM_PARITY_OUT=<file> every case appends its largest errors, as fractions of these bounds, to that file
(profiles/r12/normalize_parity.txt)."""
import functools
import os

import numpy as np
import pytest
import torch

import normalize_reference as R
from policy_checks import DEV

from quadruped_gym_amd.normalize import DeviceVecNormalize, RunningNormalizer

pytestmark = pytest.mark.gpu
STEPS = 6
# Not the defaults: an outlier among N rows that enter the statistics lies at most sqrt(N) standard deviations out, and the small
# shapes have seen fewer than 100 rows when the outliers come (steps 4 and 5), so a clip of 10 could not be met there.
CLIP_OBS, CLIP_REWARD = 5.0, 3.0
IDS = [f"{n}x{D}" for n, D in R.SHAPES]


def _record(line):
    print(line)
    out = os.environ.get("QG_NORM_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


@functools.lru_cache(maxsize=None)
def _data(n, D):
    """Six steps of inputs (read-only): observations of every column kind, rewards, and dones on about one env in five."""
    rng = np.random.default_rng(1000 * n + D)
    obs = [R.columns(rng, n, D, k) for k in range(STEPS)]
    rew = [(0.5 + rng.standard_normal(n)).astype(np.float32) for _ in range(STEPS)]
    for k in (4, 5):
        rew[k][(3 * k) % n] = 60.0                          # beyond the reward clip once the statistic has seen enough rows
    done = [(rng.random(n) < 0.2).astype(np.uint8) for _ in range(STEPS)]
    for a in obs + rew + done:
        a.setflags(write=False)
    return obs, rew, done


@functools.lru_cache(maxsize=None)
def _checker(n, D):
    """The checker's state after each of the six steps, and the largest |return| its statistic has seen by then (the returns
    before the dones cleared them)."""
    obs, rew, done = _data(n, D)
    nz = R.Normalizer(n, D, clip_obs=CLIP_OBS, clip_reward=CLIP_REWARD)
    states, ret_seen, biggest = [], [], 0.0
    for k in range(STEPS):
        biggest = max(biggest, float(np.abs(nz.returns * nz.gamma + rew[k].astype(np.float64)).max()))
        nz.step(obs[k], rew[k], done[k])
        states.append(nz.state())
        ret_seen.append(biggest)
    return states, ret_seen


def _check_statistics(got, ref, seen, ret_seen, what):
    """The statistics rule of the module docstring; returns the largest errors as fractions of their bounds."""
    assert got["obs_rms.count"] == ref["obs_rms.count"] and got["ret_rms.count"] == ref["ret_rms.count"], what
    m_tol = 1e-12 * seen
    v_tol = 1e-9 * ref["obs_rms.var"] + m_tol ** 2
    dm, dv = np.abs(got["obs_rms.mean"] - ref["obs_rms.mean"]), np.abs(got["obs_rms.var"] - ref["obs_rms.var"])
    fm = np.divide(dm, m_tol, out=np.where(dm > 0, np.inf, 0.0), where=m_tol > 0)
    fv = dv / v_tol
    assert np.all(dm <= m_tol), f"{what}: mean at {fm.max():.3g} of the bound (column {int(np.argmax(fm))})"
    assert np.all(dv <= v_tol), f"{what}: var at {fv.max():.3g} of the bound (column {int(np.argmax(fv))})"
    # the variance has the unit of a squared return: the tighter of the two readings of "relative to the largest |return|"
    r_tol, rv_tol = 1e-12 * ret_seen, 1e-12 * min(ret_seen, ret_seen ** 2)
    dr = max(float(np.abs(got["returns"] - ref["returns"]).max()), abs(float(got["ret_rms.mean"] - ref["ret_rms.mean"])))
    drv = abs(float(got["ret_rms.var"] - ref["ret_rms.var"]))
    assert dr <= r_tol and drv <= rv_tol, f"{what}: returns off by {dr:.3g} (bound {r_tol:.3g}), their variance by {drv:.3g} (bound {rv_tol:.3g})"
    fr = max(dr / r_tol, drv / rv_tol) if ret_seen > 0 else 0.0
    return float(fm.max()), float(fv.max()), fr


def _new(n, D, **kw):
    return RunningNormalizer(n, D, clip_obs=CLIP_OBS, clip_reward=CLIP_REWARD, **kw)


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)            # a copy: the shared inputs are read-only


def _state_bytes(nz):
    sd = nz.state_dict()
    return b"".join(np.asarray(sd[k], np.float64).tobytes() for k in sorted(sd))


@functools.lru_cache(maxsize=None)
def _eager(n, D):
    """Six eager training steps from a fresh handle, out of place: per step the outputs and the state the device reports."""
    obs, rew, done = _data(n, D)
    nz = _new(n, D)
    outs, states = [], []
    for k in range(STEPS):
        o, r = torch.empty((n, D), device=DEV), torch.empty(n, device=DEV)
        nz.step(_t(obs[k]), _t(rew[k]), _t(done[k]), obs_out=o, reward_out=r)
        states.append(nz.state_dict())
        outs.append((o.cpu().numpy(), r.cpu().numpy()))
    final = _state_bytes(nz)
    nz.close()
    return outs, states, final


def _check_outputs(out, x, mean, var, epsilon, clip, what):
    """The output rule; returns the largest error in ulps."""
    ref = R.apply_f64(x, mean, var, epsilon)
    over = np.abs(ref) > clip * (1 + 1e-6)
    assert np.all(np.abs(out) <= np.float32(clip)), what
    assert np.array_equal(out[over], (np.sign(ref[over]) * clip).astype(np.float32)), f"{what}: clipped elements are not exactly at the clip"
    refc = np.clip(ref, -clip, clip)
    err = np.abs(out.astype(np.float64) - refc) / R.ulp32(refc)
    assert err.max() <= 1.0, f"{what}: {err.max():.3f} ulp"
    return float(err.max()), int(over.sum())


# ---- 1. statistics against the checker ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", R.SHAPES, ids=IDS)
def test_statistics_after_six_training_steps(n, D):
    obs, rew, done = _data(n, D)
    _, states, _ = _eager(n, D)
    want, ret_seen = _checker(n, D)
    seen = np.zeros(D)
    worst_m = worst_v = worst_r = 0.0
    for k in range(STEPS):
        seen = np.maximum(seen, np.abs(obs[k].astype(np.float64)).max(0))
        fm, fv, fr = _check_statistics(states[k], want[k], seen, ret_seen[k], f"step {k}")
        worst_m, worst_v, worst_r = max(worst_m, fm), max(worst_v, fv), max(worst_r, fr)
    _record(f"statistics {n}x{D}: mean {worst_m:.3g} of its bound, var {worst_v:.3g}, returns {worst_r:.3g}")


# ---- 2. outputs against the formula with the device's own statistics -------------------------------------------------------------------
@pytest.mark.parametrize("n,D", R.SHAPES, ids=IDS)
def test_outputs_within_one_ulp_and_clipped_exactly(n, D):
    obs, rew, done = _data(n, D)
    outs, states, _ = _eager(n, D)
    worst_o = worst_r = 0.0
    clipped = clipped_r = 0
    for k in range(STEPS):
        sd = states[k]
        e, c = _check_outputs(outs[k][0], obs[k], sd["obs_rms.mean"], sd["obs_rms.var"], 1e-8, CLIP_OBS, f"obs, step {k}")
        worst_o, clipped = max(worst_o, e), clipped + c
        e, c = _check_outputs(outs[k][1], rew[k], 0.0, sd["ret_rms.var"], 1e-8, CLIP_REWARD, f"reward, step {k}")
        worst_r, clipped_r = max(worst_r, e), clipped_r + c
    if D >= len(R.COLUMN_KINDS) and n >= 17:
        assert clipped > 0 and clipped_r > 0                # the test did meet both clips
    _record(f"outputs {n}x{D}: obs {worst_o:.3f} ulp, reward {worst_r:.3f} ulp, {clipped} + {clipped_r} clipped")


@pytest.mark.parametrize("n,D", [(17, 33), (83, 260)], ids=["17x33", "83x260"])
def test_a_step_with_training_off_changes_no_word_of_the_state(n, D):
    obs, rew, done = _data(n, D)
    nz = _new(n, D)
    for k in range(3):
        nz.step(_t(obs[k]), _t(rew[k]), _t(done[k]), obs_out=torch.empty((n, D), device=DEV), reward_out=torch.empty(n, device=DEV))
    before, sd = _state_bytes(nz), nz.state_dict()
    nz.training = False
    o, r = torch.empty((n, D), device=DEV), torch.empty(n, device=DEV)
    nz.step(_t(obs[3]), _t(rew[3]), _t(np.ones(n, np.uint8)), obs_out=o, reward_out=r)
    assert _state_bytes(nz) == before
    _check_outputs(o.cpu().numpy(), obs[3], sd["obs_rms.mean"], sd["obs_rms.var"], 1e-8, CLIP_OBS, "obs, training off")
    _check_outputs(r.cpu().numpy(), rew[3], 0.0, sd["ret_rms.var"], 1e-8, CLIP_REWARD, "reward, training off")
    nz.close()


def test_switched_off_flags_copy_through_and_state_round_trips():
    n, D = 83, 26
    obs, rew, done = _data(n, D)
    nz = _new(n, D, norm_obs=False, norm_reward=False)
    o, r = torch.empty((n, D), device=DEV), torch.empty(n, device=DEV)
    nz.step(_t(obs[0]), _t(rew[0]), _t(done[0]), obs_out=o, reward_out=r)
    assert np.array_equal(o.cpu().numpy(), obs[0]) and np.array_equal(r.cpu().numpy(), rew[0])
    sd = nz.state_dict()
    assert np.array_equal(sd["obs_rms.mean"], np.zeros(D)) and sd["obs_rms.count"] == 1e-4 and sd["ret_rms.count"] == 1e-4 + n
    nz.close()
    # set_state / get_state: exact, and a restored handle continues with the bits of the original
    a, b = _new(n, D), _new(n, D)
    for k in range(2):
        a.step(_t(obs[k]), _t(rew[k]), _t(done[k]), obs_out=o, reward_out=r)
    b.load_state_dict(a.state_dict())
    assert _state_bytes(a) == _state_bytes(b)
    oa, ob = torch.empty((n, D), device=DEV), torch.empty((n, D), device=DEV)
    a.training = b.training = False
    a.step(_t(obs[2]), obs_out=oa)
    b.step(_t(obs[2]), obs_out=ob)
    assert torch.equal(oa, ob)
    a.close(), b.close()


def test_a_single_column_at_an_inner_stride_equals_its_contiguous_copy():
    """obs_dim 1: the [5, 1] view x[:, ::2] of a [5, 2] tensor (strides (2, 2)) has no inner stride to violate -- the library takes
    the row stride alone -- and so does an output of the same kind."""
    n = 5
    rng = np.random.default_rng(7)
    x = _t(rng.normal(2.0, 3.0, (3, n, 2)).astype(np.float32))
    rew, done = _t(rng.normal(0.0, 1.0, (3, n)).astype(np.float32)), _t((rng.random((3, n)) < 0.4).astype(np.uint8))
    x0 = x.clone()
    a, b = _new(n, 1), _new(n, 1)
    for k in range(3):
        wide = torch.full((n, 2), -7.0, device=DEV)
        view, out = x[k][:, ::2], wide[:, ::2]
        assert tuple(view.shape) == (n, 1) and view.stride() == (2, 2) == out.stride()
        ra, rb = torch.empty(n, device=DEV), torch.empty(n, device=DEV)
        a.step(view, rew[k], done[k], obs_out=out, reward_out=ra)
        ob, _ = b.step(view.contiguous(), rew[k], done[k], obs_out=torch.empty((n, 1), device=DEV), reward_out=rb)
        assert torch.equal(out, ob) and torch.equal(ra, rb)
        assert torch.equal(wide[:, 1], torch.full((n,), -7.0, device=DEV))          # the column between the output's rows
        assert _state_bytes(a) == _state_bytes(b)
    assert torch.equal(x, x0)                                                       # the inputs, the odd column included
    a.close(), b.close()


# ---- 3. bit-for-bit identity: run to run, eager against graph replay ---------------------------------------------------------------------
@pytest.mark.parametrize("n,D", R.SHAPES, ids=IDS)
def test_two_runs_and_both_graph_forms_leave_the_same_bits(n, D):
    obs, rew, done = _data(n, D)
    outs, _, final = _eager(n, D)
    want = [np.concatenate([o.ravel(), r]) for o, r in outs]

    # a second run from a fresh handle, on a side stream
    side = torch.cuda.Stream(DEV)
    t_obs, t_rew, t_done = [_t(a) for a in obs], [_t(a) for a in rew], [_t(a) for a in done]
    o = [torch.empty((n, D), device=DEV) for _ in range(STEPS)]
    r = [torch.empty(n, device=DEV) for _ in range(STEPS)]
    torch.cuda.synchronize()

    def run(nz, stream=None):
        for k in range(STEPS):
            nz.step(t_obs[k], t_rew[k], t_done[k], obs_out=o[k], reward_out=r[k], stream=stream)

    def collect():
        torch.cuda.synchronize()
        got = [np.concatenate([o[k].cpu().numpy().ravel(), r[k].cpu().numpy()]) for k in range(STEPS)]
        for t in o + r:
            t.zero_()
        torch.cuda.synchronize()
        return got

    nz = _new(n, D)
    run(nz, side)
    got = collect()
    assert _state_bytes(nz) == final and all(np.array_equal(a, b) for a, b in zip(got, want))
    nz.close()

    # one replay of a six-step graph (a single stream, no parallel branches)
    nz = _new(n, D)
    fresh = nz.state_dict()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run(nz)
    nz.load_state_dict(fresh)                               # whatever a capture may have run, start from the fresh state
    for t in o + r:
        t.zero_()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        graph.replay()
    got = collect()
    assert _state_bytes(nz) == final and all(np.array_equal(a, b) for a, b in zip(got, want))
    nz.close()

    # six replays of a one-step graph: the inputs change in static buffers, everything else lives on the device
    nz = _new(n, D)
    s_obs, s_rew, s_done = torch.zeros((n, D), device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV, dtype=torch.uint8)
    s_o, s_r = torch.zeros((n, D), device=DEV), torch.zeros(n, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        nz.step(s_obs, s_rew, s_done, obs_out=s_o, reward_out=s_r)
    nz.load_state_dict(fresh)
    got = []
    for k in range(STEPS):
        with torch.cuda.stream(side):
            s_obs.copy_(t_obs[k]), s_rew.copy_(t_rew[k]), s_done.copy_(t_done[k])
            graph.replay()
        side.synchronize()
        got.append(np.concatenate([s_o.cpu().numpy().ravel(), s_r.cpu().numpy()]))
    assert _state_bytes(nz) == final and all(np.array_equal(a, b) for a, b in zip(got, want))
    nz.close()


# ---- 4. a row's output depends on the statistics and that row alone ----------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(17, 33), (83, 260), (83, 512)], ids=["17x33", "83x260", "83x512"])
def test_apply_is_row_independent(n, D):
    obs, rew, done = _data(n, D)
    nz = _new(n, D)
    nz.update_obs(_t(obs[0]))
    nz.update_obs(_t(obs[1][:11]))                          # any n >= 1
    x = _t(obs[2])
    whole = nz.normalize_obs(x, out=torch.empty_like(x))
    one = nz.normalize_obs(x[5:6], out=torch.empty((1, D), device=DEV))
    wide = torch.full((n, D + 3), 7.0, device=DEV)          # an odd row stride, off the 16-byte path
    wide[:, 1:D + 1] = x
    odd = nz.normalize_obs(wide[:, 1:D + 1], out=torch.empty_like(x))
    inplace = nz.normalize_obs(wide[:, 1:D + 1])
    torch.cuda.synchronize()
    assert torch.equal(whole[5:6], one) and torch.equal(whole, odd) and torch.equal(whole, inplace)
    assert bool((wide[:, 0] == 7.0).all()) and bool((wide[:, D + 1:] == 7.0).all())      # nothing beside the rows was written
    sd = nz.state_dict()
    ref = R.RunningMeanStd((D,))
    ref.update(obs[0]), ref.update(obs[1][:11])
    assert sd["obs_rms.count"] == ref.count and sd["ret_rms.count"] == 1e-4
    _check_outputs(whole.cpu().numpy(), obs[2], sd["obs_rms.mean"], sd["obs_rms.var"], 1e-8, CLIP_OBS, "apply")
    nz.close()


# ---- 5. in place, packed, and the two kinds of done --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", [(17, 33), (83, 26), (83, 260)], ids=["17x33", "83x26", "83x260"])
def test_in_place_packed_and_float_done_equal_the_plain_form(n, D):
    obs, rew, done = _data(n, D)
    outs, _, final = _eager(n, D)
    a, b, c = _new(n, D), _new(n, D), _new(n, D)
    for k in range(STEPS):
        # in place, done as uint8
        o, r = _t(obs[k]), _t(rew[k])
        ro, rr = a.step(o, r, _t(done[k]))
        assert ro is o and rr is r
        # packed rows in place (stride D + 2, done as float32 in the last column)
        packed = torch.cat([_t(obs[k]), _t(rew[k])[:, None], _t(done[k]).float()[:, None]], dim=1).contiguous()
        assert b.step_packed(packed) is packed
        # three pointers, done as float32, out of place
        o3, r3 = torch.empty((n, D), device=DEV), torch.empty(n, device=DEV)
        c.step(_t(obs[k]), _t(rew[k]), _t(done[k]).float(), obs_out=o3, reward_out=r3)
        torch.cuda.synchronize()
        want_o, want_r = outs[k]
        assert np.array_equal(o.cpu().numpy(), want_o) and np.array_equal(r.cpu().numpy(), want_r)
        assert np.array_equal(packed[:, :D].cpu().numpy(), want_o) and np.array_equal(packed[:, D].cpu().numpy(), want_r)
        assert np.array_equal(packed[:, D + 1].cpu().numpy(), done[k].astype(np.float32))
        assert np.array_equal(o3.cpu().numpy(), want_o) and np.array_equal(r3.cpu().numpy(), want_r)
    assert _state_bytes(a) == final and _state_bytes(b) == final and _state_bytes(c) == final
    # packed, out of place: the done column travels too
    src = torch.cat([_t(obs[0]), _t(rew[0])[:, None], _t(done[0]).float()[:, None]], dim=1).contiguous()
    keep, dst = src.clone(), torch.zeros_like(src)
    a.training = b.training = False
    b.step_packed(src, out=dst)
    a.step_packed(keep)
    assert torch.equal(dst, keep)
    for nz in (a, b, c):
        nz.close()


# ---- 6. the wrapper -------------------------------------------------------------------------------------------------------------------------
def _envs(kind):
    from quadruped_gym_amd.envs.vec_env import QuadrupedVecEnv
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv, WalkingQuadrupedVecEnv
    if kind == "plain":
        kw = dict(reward_fns={"forward": 1.0, "control_cost": -0.1, "alive_bonus": 1.0}, termination_fns={"fall": 0.05}, max_time=0.05)
        return QuadrupedVecEnv(64, **kw), QuadrupedVecEnv(64, **kw)
    kw = dict(random_controls=True, random_init=True, device_commands=True, reset_options={"min_speed": 0.0, "max_speed": 0.5},
              max_time=0.05, nan_direction=False)
    if kind == "walking":
        return WalkingQuadrupedVecEnv(64, **kw), WalkingQuadrupedVecEnv(64, **kw)
    return POWalkingQuadrupedVecEnv(64, obs_window=10, **kw), POWalkingQuadrupedVecEnv(64, obs_window=10, **kw)


@pytest.mark.parametrize("kind", ["plain", "walking", "po"])
def test_wrapper_equals_the_env_followed_by_the_checker(kind):
    n, steps = 64, 10
    inner, twin = _envs(kind)
    env = DeviceVecNormalize(inner)
    D = env.normalizer.obs_dim
    ref = R.Normalizer(n, D)
    # reset(): the observation statistics take the reset rows, the returns are cleared
    first = env.reset()
    raw0 = twin.reset()
    ref.reset_returns()
    ref.update_obs(raw0)
    seen, ret_seen = np.abs(raw0.astype(np.float64)).max(0), 0.0
    sd = env.normalizer.state_dict()
    assert np.array_equal(env.get_original_obs(), raw0)
    _check_outputs(first, raw0, sd["obs_rms.mean"], sd["obs_rms.var"], 1e-8, 10.0, "reset")
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    acts = torch.rand((steps, n, 12), generator=gen, device=DEV) * 2 - 1
    mk = lambda *s, dt=torch.float32: torch.zeros(s, device=DEV, dtype=dt)     # noqa: E731
    finished = 0
    snap, later = None, []
    for k in range(steps + 3):
        if k == steps:                                      # snapshot() -> three steps -> restore() -> the same three steps
            env.restore(snap)
        a = acts[k if k < steps else k - 3]
        if kind == "plain":
            got = env.step_tensor(a).clone()
            raw = twin.step_tensor(a).clone() if k < steps else None
            g_obs, g_rew = got[:, :D], got[:, D]
            if raw is not None:
                assert torch.equal(got[:, D + 1], raw[:, D + 1])
                r_obs, r_rew, r_done = raw[:, :D].cpu().numpy(), raw[:, D].cpu().numpy(), raw[:, D + 1].cpu().numpy()
            g_term = r_term = None
        else:
            bufs = [(mk(n, D), mk(n), mk(n, dt=torch.uint8), mk(n, D)) for _ in range(2)]
            po = {"terminal_obs": bufs[0][3]} if kind == "po" else {}
            env.step_tensor(a, bufs[0][0], bufs[0][1], bufs[0][2], **po)
            g_obs, g_rew, g_term = bufs[0][0], bufs[0][1], (bufs[0][3] if kind == "po" else None)
            if k < steps:
                po = {"terminal_obs": bufs[1][3]} if kind == "po" else {}
                twin.step_tensor(a, bufs[1][0], bufs[1][1], bufs[1][2], **po)
                assert torch.equal(bufs[0][2], bufs[1][2])
                r_obs, r_rew, r_done = bufs[1][0].cpu().numpy(), bufs[1][1].cpu().numpy(), bufs[1][2].cpu().numpy()
                r_term = bufs[1][3].cpu().numpy() if kind == "po" else None
        torch.cuda.synchronize()
        bits = (g_obs.cpu().numpy().tobytes(), g_rew.cpu().numpy().tobytes(), _state_bytes(env.normalizer))
        if k >= steps:
            assert bits == later[k - steps], f"step {k - steps} after restore() differs"
            continue
        if k >= steps - 3:
            later.append(bits)
        assert np.isfinite(r_obs).all() and np.isfinite(r_rew).all()
        seen = np.maximum(seen, np.abs(r_obs.astype(np.float64)).max(0))
        ret_seen = max(ret_seen, float(np.abs(ref.returns * ref.gamma + r_rew.astype(np.float64)).max()))
        ref.step(r_obs, r_rew, r_done)
        finished += int((r_done != 0).sum())
        sd = env.normalizer.state_dict()
        _check_statistics(sd, ref.state(), seen, ret_seen, f"{kind}, step {k}")
        _check_outputs(g_obs.cpu().numpy(), r_obs, sd["obs_rms.mean"], sd["obs_rms.var"], 1e-8, 10.0, f"{kind} obs, step {k}")
        _check_outputs(g_rew.cpu().numpy(), r_rew, 0.0, sd["ret_rms.var"], 1e-8, 10.0, f"{kind} reward, step {k}")
        if g_term is not None:
            rows = r_done != 0
            if rows.any():
                _check_outputs(g_term.cpu().numpy()[rows], r_term[rows], sd["obs_rms.mean"], sd["obs_rms.var"], 1e-8, 10.0,
                               f"{kind} terminal")
        if k == steps - 4:
            snap = env.snapshot()
    assert finished > 0                                     # episodes did end: the dones cleared returns along the way
    assert env.num_envs == n and env.action_space is inner.action_space      # everything else passes through
    env.close(), twin.close()


def test_a_normalised_packed_row_feeds_the_fused_policy():
    from quadruped_gym_amd.envs.vec_env import QuadrupedVecEnv
    from quadruped_gym_amd.policy import FusedMlpPolicy
    n = 64
    env = DeviceVecNormalize(QuadrupedVecEnv(n, reward_fns={"forward": 1.0, "alive_bonus": 1.0}, termination_fns={"fall": 0.05}))
    env.venv.reset()
    pol = FusedMlpPolicy(33, (64, 64), 12)
    rng = np.random.default_rng(9)
    pol.set_params((0.1 * rng.standard_normal(pol.n_params)).astype(np.float32))
    acts, val = torch.zeros((n, 12), device=DEV), torch.zeros(n, device=DEV)
    for _ in range(3):
        packed = env.step_tensor(acts)
        pol.forward(packed[:, :33], acts, value=val)        # the normalised rows, read in place at stride 35
    torch.cuda.synchronize()
    assert torch.isfinite(packed).all() and torch.isfinite(acts).all() and float(acts.abs().max()) > 0
    assert float(packed[:, :33].abs().max()) <= 10.0
    pol.close(), env.close()
