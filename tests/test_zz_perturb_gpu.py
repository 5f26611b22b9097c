"""The perturbation layer on the GPU (qg_perturb_*, csrc/qg_perturb.hip) against the float64 checker of tests/perturb_reference.py.

Integers (delays, ages, episodes) exactly; delayed actions, zero-std columns, the travel of a frame through the stack, graph replay,
shards and restored state bit for bit; noise terms within  4 E_z (obs_std[c] + bias_std[c]) + 2^-23 (|in| + |e|)  of the checker
(E_z: perturb_reference.error_budget, measured on a float32 NumPy evaluation); the GPU's own draws within the moment
bounds the checker's passed (tests/test_perturb_reference.py).  With QG_PERTURB_PARITY_OUT=<file> the cases append their largest
errors as fractions of the bound to that file (profiles/r24/perturb_parity.txt).
The module's name puts it last in collection: it leaves the process state of the modules before it as it was."""
import os

import numpy as np
import pytest
import torch

import perturb_reference as R
from policy_checks import DEV

from quadruped_gym_amd.perturb import DevicePerturbedVecEnv, Perturbation

pytestmark = pytest.mark.gpu
SHAPE_IDS = [f"{n}x{W}x{F}" for n, W, F in R.SHAPES]
DELAY_IDS = [f"max{m}-{lo}to{hi}" for m, (lo, hi) in R.DELAYS]
SEED = 11


def _record(line):
    print(line)
    out = os.environ.get("QG_PERTURB_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def _t(a, dtype=None):
    t = torch.tensor(np.asarray(a)).to(DEV)                  # a copy: the shared inputs stay as they are
    return t if dtype is None else t.to(dtype)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _pair(n, W, F, max_delay=0, delays=(0, 0), action_std=0.0, noisy=True, done_row="terminal", base=0, n_handle=None):
    """A handle and its checker.  `n_handle` < n: the handle (and the checker) cover the envs [n - n_handle, n) of an n-env run."""
    obs_std, bias_std = R.column_stds(F) if noisy else (None, None)
    m = n if n_handle is None else n_handle
    kw = dict(max_delay=max_delay, delays=delays, action_std=action_std, obs_std=obs_std, bias_std=bias_std, done_row=done_row, seed=SEED,
              env_index_base=base + n - m)
    return Perturbation(m, F, W, reset_action=R.RESET_ACTION, device=0, **kw), R.Checker(m, F, W, reset_action=R.RESET_ACTION, **kw)


# ---- 1. latency ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_delay,delays", R.DELAYS, ids=DELAY_IDS)
@pytest.mark.parametrize("n,W,F", R.SHAPES, ids=SHAPE_IDS)
def test_delayed_actions_are_bit_copies(n, W, F, max_delay, delays):
    """action_std = 0: the delays are the checker's integers and every output row is the input row of d_i steps earlier in the same
    episode, or reset_action -- by its bits.  In place as well (actions_out == actions_in)."""
    pz, ck = _pair(n, W, F, max_delay, delays, noisy=False)
    acts, done = R.rows(n, R.NJ, tag=1), R.done_table(n)
    zeros = torch.zeros((n, W * F), device=DEV)
    history = {}                                             # (env, episode, age) -> the row the policy wrote
    for t in range(R.STEPS):
        d = pz.delays()
        assert np.array_equal(d, ck.delays()) and d.min() >= delays[0] and d.max() <= delays[1]
        for i in range(n):
            history[(i, int(ck.episode[i]), int(ck.age[i]))] = acts[t, i]
        want = np.stack([history.get((i, int(ck.episode[i]), int(ck.age[i]) - int(d[i])), np.asarray(R.RESET_ACTION, np.float32)) for i in range(n)])
        _, v, _ = ck.perturb_actions(acts[t])
        assert np.array_equal(v.view(np.uint32), want.view(np.uint32))          # the checker's ring is that history
        a_in = _t(acts[t])
        out = pz.perturb_actions(a_in, out=torch.empty_like(a_in))
        assert np.array_equal(_bits(out), want.view(np.uint32)) and np.array_equal(_bits(a_in), acts[t].view(np.uint32))
        if t % 2:                                            # the same call again, in place: the ring slot takes the same row
            assert np.array_equal(_bits(pz.perturb_actions(a_in)), want.view(np.uint32))
        pz.observe(zeros, _t(done[t]))
        ck.observe(zeros.cpu().numpy(), done[t])
    st = pz.state()
    assert np.array_equal(st["age"], ck.age) and np.array_equal(st["episode"], ck.episode)
    assert np.array_equal(st["ring"].view(np.uint32), ck.ring.view(np.uint32))
    pz.close()


# ---- 2. the stack property ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("done_row", ["reset", "terminal"])
@pytest.mark.parametrize("n,W,F", R.SHAPES, ids=SHAPE_IDS)
def test_a_frame_keeps_its_noise_through_the_stack(n, W, F, done_row):
    """All-zero input rows: out[t][slot k] == out[t - 1][slot k + 1] bit for bit within an episode; a finished env's row and its
    terminal_obs carry the right episode's terms."""
    pz, ck = _pair(n, W, F, done_row=done_row)
    done = R.done_table(n)
    prev = None
    for t in range(R.STEPS):
        fin = done[t].astype(bool)
        obs = torch.zeros((n, W * F), device=DEV)
        term = torch.zeros((n, W * F), device=DEV) if done_row == "reset" else None
        pz.observe(obs, _t(done[t]).bool() if t % 2 else _t(done[t]), terminal_obs=term)
        want = ck.observe(np.zeros((n, W * F)), done[t], terminal=None if term is None else np.zeros((n, W * F)))
        got = _bits(obs).reshape(n, W, F)
        assert float(np.abs(obs.cpu().numpy() - want["ref"]).max()) <= 4 * R.error_budget() * 0.3 + 2.0 ** -22
        if prev is not None:
            same_episode = ~fin if done_row == "reset" else np.ones(n, bool)       # a terminal row still belongs to the old episode
            same_episode &= ~done[t - 1].astype(bool) | (done_row == "reset")      # ... and the row after it to the new one
            assert np.array_equal(got[same_episode, :-1], prev[same_episode, 1:])
            if done_row == "terminal" and done[t - 1].any():                        # first row of an episode whose reset frame was never shown
                first = done[t - 1].astype(bool)
                assert np.all(got[first][:, :-1] == got[first][:, :1]) and (W == 1 or not np.array_equal(got[first, :-1], prev[first, 1:]))
        if done_row == "reset" and fin.any():
            assert np.all(got[fin] == got[fin][:, :1])                              # frame 0 of the new episode in every slot
            tb = _bits(term).reshape(n, W, F)
            assert not tb[~fin].any()                                               # live envs' terminal rows are not touched
            assert float(np.abs(term.cpu().numpy() - want["term_ref"])[fin].max()) <= 4 * R.error_budget() * 0.3 + 2.0 ** -22
            if prev is not None:
                assert np.array_equal(tb[fin, :-1], prev[fin, 1:])
        prev = got
    assert np.array_equal(pz.state()["episode"], ck.episode) and np.array_equal(pz.state()["age"], ck.age)
    pz.close()


# ---- 3. parity with the float64 checker ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("done_row", ["reset", "terminal"])
@pytest.mark.parametrize("n,W,F", R.SHAPES, ids=SHAPE_IDS)
def test_noise_matches_the_checker(n, W, F, done_row):
    """Random rows, in place, at a row stride wider than the row; done as float32 at a stride (a packed row's column).  Every
    element within the bound of the module docstring; zero-std columns keep their bits; the words between the rows are not written."""
    max_delay, delays = R.DELAYS[1]
    pz, ck = _pair(n, W, F, max_delay, delays, action_std=0.05, done_row=done_row)
    obs_std, bias_std = R.column_stds(F)
    std_sum = np.tile((obs_std + bias_std).astype(np.float64), W)
    quiet = np.tile((obs_std == 0) & (bias_std == 0), W)
    assert quiet.any() and (~quiet).any()
    D, pad = W * F, 3
    rows, terms, acts, done = R.rows(n, D, tag=2), R.rows(n, D, tag=3), R.rows(n, R.NJ, tag=4), R.done_table(n)
    worst = {"obs": 0.0, "terminal": 0.0, "action": 0.0}
    for t in range(R.STEPS):
        a_want, _, a_e = ck.perturb_actions(acts[t])
        a_out = pz.perturb_actions(_t(acts[t]))
        bound = 4 * R.error_budget() * 0.05 + 2.0 ** -23 * (np.abs(a_want - a_e) + np.abs(a_e))
        err = np.abs(a_out.cpu().numpy().astype(np.float64) - a_want)
        worst["action"] = max(worst["action"], float((err / bound).max()))
        assert np.all(err <= bound)

        wide = torch.full((n, D + pad + 2), 7.0, device=DEV)
        wide[:, :D] = _t(rows[t])
        wide[:, D + pad + 1] = _t(done[t], torch.float32)
        term = _t(terms[t]) if done_row == "reset" else None
        pz.observe(wide[:, :D], wide[:, D + pad + 1], terminal_obs=term)
        want = ck.observe(rows[t], done[t], terminal=terms[t] if term is not None else None)
        got = wide.cpu().numpy()
        assert np.all(got[:, D:D + pad + 1] == 7.0) and np.array_equal(got[:, D + pad + 1], done[t].astype(np.float32))
        assert np.array_equal(got[:, :D].view(np.uint32)[:, quiet], rows[t].view(np.uint32)[:, quiet])
        checks = [("obs", got[:, :D], rows[t], want["ref"], want["e"], np.ones(n, bool))]
        if term is not None:
            fin = done[t].astype(bool)
            tg = term.cpu().numpy()
            assert np.array_equal(tg.view(np.uint32)[~fin], terms[t].view(np.uint32)[~fin])
            assert np.array_equal(tg.view(np.uint32)[:, quiet], terms[t].view(np.uint32)[:, quiet])
            checks.append(("terminal", tg, terms[t], want["term_ref"], want["term_e"], fin))
        for what, g, x, ref, e, sel in checks:
            if sel.any():
                bound = R.tolerance(std_sum, x.astype(np.float64), e)
                err = np.abs(g.astype(np.float64) - ref)
                worst[what] = max(worst[what], float((err[sel][:, ~quiet] / bound[sel][:, ~quiet]).max()))
                assert np.all(err[sel] <= bound[sel]), (what, t)
    _record(f"parity {n}x{W}x{F} {done_row:8s}: worst error / bound  obs {worst['obs']:.3f}  terminal {worst['terminal']:.3f}  action {worst['action']:.3f}"
            f"  (E_z {R.error_budget():.3e})")
    pz.close()


# ---- 4. the GPU's own draws ---------------------------------------------------------------------------------------------------------------
def _at_episode(pz, ep):
    st = pz.state()
    st["episode"][:] = ep
    pz.load_state(st)


@pytest.mark.parametrize("seed", R.MOMENT_SEEDS)
def test_gpu_draws_have_standard_moments(seed):
    """The samples of tests/test_perturb_reference.py as the kernels draw them (std 1 on zero rows): the same moment bounds, and each
    draw within 4 E_z of the float64 value."""
    E, Fr, Cn = R.MOMENT_ENVS, R.MOMENT_FRAMES, R.MOMENT_COLS
    for ep in R.MOMENT_EPISODES:
        # a window of two shows frame 0 (slot 0 of the first step) beside the frames 1 .. 63
        pz = Perturbation(E, Cn, 2, obs_std=1.0, action_std=1.0, reset_action=[0.0] * 12, seed=seed, device=0)
        _at_episode(pz, ep)
        obs, act = np.empty((E, Fr, Cn)), np.empty((E, Fr, R.NJ))
        for f in range(Fr):
            act[:, f] = pz.perturb_actions(torch.zeros((E, R.NJ), device=DEV)).cpu().numpy()
            row = pz.observe(torch.zeros((E, 2 * Cn), device=DEV)).cpu().numpy().reshape(E, 2, Cn)
            if f == 0:
                obs[:, 0] = row[:, 0]
            if f + 1 < Fr:
                obs[:, f + 1] = row[:, 1]
        pz.close()
        pb = Perturbation(R.BIAS_ENVS, Cn, 1, bias_std=1.0, seed=seed, device=0)
        _at_episode(pb, ep)
        bias = pb.observe(torch.zeros((R.BIAS_ENVS, Cn), device=DEV)).cpu().numpy()
        pb.close()
        for name, got, sample in (("obs", obs, R.obs_sample), ("action", act, R.action_sample), ("bias", bias, R.bias_sample)):
            m = R.assert_moments(got, (name, seed, ep))
            dev = float(np.abs(got - sample(seed, ep)).max())
            _record(f"gpu draws {name:6s} seed {seed:5d} episode {ep}: |mean| {m[0]:.4f} |std-1| {m[1]:.4f} lag-1 {m[2]:.4f}  max |z - z64| {dev:.3e}")
            assert dev <= 4 * R.error_budget()
    lo, hi = R.DELAY_RANGE
    pd = Perturbation(R.DELAY_ENVS, 4, 1, delays=(lo, hi), seed=seed, device=0)
    d = pd.delays()
    pd.close()
    assert np.array_equal(d, R.delay_of(seed, np.arange(R.DELAY_ENVS), 0, lo, hi))
    assert np.all(np.abs(np.bincount(d, minlength=4) - R.DELAY_ENVS / 4) <= 4 * np.sqrt(R.DELAY_ENVS * 0.25 * 0.75))


# ---- 5. graph replay, shards, state, begin ------------------------------------------------------------------------------------------------
def _run(pz, n, D, steps, rows, acts, done, start=0):
    """Eager: the outputs of steps [start, start + steps) as bit patterns."""
    out = []
    for t in range(start, start + steps):
        a = pz.perturb_actions(_t(acts[t]))
        term = _t(rows[(t + 1) % R.STEPS]) if pz.done_row == "reset" else None
        o = pz.observe(_t(rows[t]), _t(done[t]), terminal_obs=term)
        out.append(np.concatenate([_bits(a).ravel(), _bits(o).ravel()] + ([_bits(term).ravel()] if term is not None else [])))
    return out


@pytest.mark.parametrize("done_row", ["reset", "terminal"])
def test_graph_replay_draws_what_eager_calls_draw(done_row):
    """One captured env-step (both launches, a single stream), replayed twelve times on changing inputs: the bits of twelve eager
    steps -- the noise is fresh at every replay because age and episode advance on the device."""
    n, W, F = R.SHAPES[1]
    max_delay, delays = R.DELAYS[1]
    D = W * F
    rows, acts, done = R.rows(n, D, tag=2), R.rows(n, R.NJ, tag=4), R.done_table(n)
    eager, _ = _pair(n, W, F, max_delay, delays, action_std=0.05, done_row=done_row)
    want = _run(eager, n, D, R.STEPS, rows, acts, done)
    eager.close()
    pz, _ = _pair(n, W, F, max_delay, delays, action_std=0.05, done_row=done_row)
    fresh = pz.state()
    s_act, s_obs, s_done = torch.zeros((n, R.NJ), device=DEV), torch.zeros((n, D), device=DEV), torch.zeros(n, device=DEV, dtype=torch.uint8)
    s_term = torch.zeros((n, D), device=DEV) if done_row == "reset" else None
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pz.perturb_actions(s_act)
        pz.observe(s_obs, s_done, terminal_obs=s_term)
    pz.load_state(fresh)                                     # whatever a capture may have run, start from the fresh state
    for t in range(R.STEPS):
        s_act.copy_(_t(acts[t])), s_obs.copy_(_t(rows[t])), s_done.copy_(_t(done[t]))
        if s_term is not None:
            s_term.copy_(_t(rows[(t + 1) % R.STEPS]))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = np.concatenate([_bits(s_act).ravel(), _bits(s_obs).ravel()] + ([_bits(s_term).ravel()] if s_term is not None else []))
        assert np.array_equal(got, want[t]), t
    assert len({w.tobytes() for w in want}) == R.STEPS
    del graph
    pz.close()


def test_a_shard_reproduces_its_rows_of_the_big_handle():
    n, W, F = R.SHAPES[1]
    max_delay, delays = R.DELAYS[1]
    D, lo = W * F, 32
    rows, acts, done = R.rows(n, D, tag=2), R.rows(n, R.NJ, tag=4), R.done_table(n)
    big, _ = _pair(n, W, F, max_delay, delays, action_std=0.05, done_row="reset")
    shard, _ = _pair(n, W, F, max_delay, delays, action_std=0.05, done_row="reset", n_handle=n - lo)
    assert shard.num_envs == 35 and shard.desc.env_index_base == lo
    assert np.array_equal(shard.delays(), big.delays()[lo:])
    for t in range(R.STEPS):
        a_big, a_sh = big.perturb_actions(_t(acts[t])), shard.perturb_actions(_t(acts[t, lo:]))
        t_big, t_sh = _t(rows[(t + 1) % R.STEPS]), _t(rows[(t + 1) % R.STEPS][lo:])
        o_big = big.observe(_t(rows[t]), _t(done[t]), terminal_obs=t_big)
        o_sh = shard.observe(_t(rows[t, lo:]), _t(done[t, lo:]), terminal_obs=t_sh)
        for b, s in ((a_big, a_sh), (o_big, o_sh), (t_big, t_sh)):
            assert np.array_equal(_bits(b)[lo:], _bits(s)), t
    big.close(), shard.close()


def test_a_restored_state_continues_bit_for_bit():
    n, W, F = R.SHAPES[1]
    max_delay, delays = R.DELAYS[1]
    D = W * F
    rows, acts, done = R.rows(n, D, tag=2), R.rows(n, R.NJ, tag=4), R.done_table(n)
    pz, _ = _pair(n, W, F, max_delay, delays, action_std=0.05, done_row="reset")
    _run(pz, n, D, 6, rows, acts, done)
    state = pz.state()
    want = _run(pz, n, D, 6, rows, acts, done, start=6)
    other, _ = _pair(n, W, F, max_delay, delays, action_std=0.05, done_row="reset")
    other.load_state(state)
    again = other.state()
    assert all(np.array_equal(again[k].view(np.uint8), state[k].view(np.uint8)) for k in ("age", "episode", "ring"))
    got = _run(other, n, D, 6, rows, acts, done, start=6)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    with pytest.raises(ValueError):
        other.load_state({**state, "age": state["age"][:-1]})
    pz.close(), other.close()


def test_begin_restarts_only_the_masked_envs():
    n, W, F = R.SHAPES[1]
    D = W * F
    pz, ck = _pair(n, W, F, 3, (0, 3), done_row="reset")
    rows, done = R.rows(n, D, tag=2), R.done_table(n)
    for t in range(3):
        pz.observe(_t(rows[t]), _t(done[t]))
        ck.observe(rows[t], done[t])
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    obs_std, bias_std = R.column_stds(F)
    std_sum = np.tile((obs_std + bias_std).astype(np.float64), W)
    for m, tag in ((mask, 5), (None, 6)):
        r = R.rows(n, D, tag=tag)[0]
        got = pz.begin(None if m is None else _t(m), _t(r)).cpu().numpy()
        want = ck.begin(m, r)
        sel = np.ones(n, bool) if m is None else m.astype(bool)
        assert np.array_equal(got.view(np.uint32)[~sel], r.view(np.uint32)[~sel])
        assert np.all(np.abs(got.astype(np.float64) - want["ref"]) <= R.tolerance(std_sum, r.astype(np.float64), want["e"]))
        st = pz.state()
        assert np.array_equal(st["age"], ck.age) and np.array_equal(st["episode"], ck.episode) and np.array_equal(pz.delays(), ck.delays())
    pz.begin()                                               # no rows: the counters alone
    ck.begin()
    assert np.array_equal(pz.state()["episode"], ck.episode) and not pz.state()["age"].any()
    with pytest.raises(ValueError):
        pz.begin(torch.zeros(n - 1, device=DEV, dtype=torch.uint8))
    with pytest.raises(ValueError):
        pz.observe(torch.zeros((n, D + 1), device=DEV))
    pz.close()


# ---- 6. through the envs ------------------------------------------------------------------------------------------------------------------
def _po_envs():
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
    kw = dict(random_controls=True, random_init=True, device_commands=True, reset_options={"min_speed": 0.0, "max_speed": 0.5}, max_time=0.04,
              nan_direction=False)
    return POWalkingQuadrupedVecEnv(8, obs_window=3, **kw), POWalkingQuadrupedVecEnv(8, obs_window=3, **kw)


@pytest.mark.parametrize("latency", [0, 1])
def test_po_env_through_the_wrapper(latency):
    """Every std zero.  Latency (0, 0): bit-identical to a twin env without the wrapper.  Latency (1, 1): bit-identical to the twin
    stepped with the actions shifted by one step, default_ctrl first and after every auto-reset.  The caller's actions stay as written."""
    inner, twin = _po_envs()
    n, D, steps = 8, inner.obs_dim, 14
    step_s = float(inner.model.opt.timestep) * inner.frame_skip
    env = DevicePerturbedVecEnv(inner, action_latency=(latency * step_s, latency * step_s), seed=3)
    assert env.perturbation.delay_range == (latency, latency) and env.perturbation.done_row == "reset"
    assert (env.perturbation.frame_dim, env.perturbation.window) == (26, 3)
    assert np.array_equal(env.reset(), twin.reset())
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    acts = torch.rand((steps, n, 12), generator=gen, device=DEV) * 2 - 1
    default = torch.tensor(list(inner._sim.task.default_ctrl), device=DEV, dtype=torch.float32)
    mk = lambda *s, dt=torch.float32: torch.zeros(s, device=DEV, dtype=dt)     # noqa: E731
    first = torch.ones(n, device=DEV, dtype=torch.bool)                        # envs at age 0
    finished = 0
    for k in range(steps):
        got, ref = [(mk(n, D), mk(n), mk(n, dt=torch.uint8), mk(n, D)) for _ in range(2)]
        a = acts[k].clone()
        env.step_tensor(a, got[0], got[1], got[2], terminal_obs=got[3])
        assert torch.equal(a, acts[k])
        shifted = acts[k] if latency == 0 else torch.where(first[:, None], default[None, :], acts[k - 1])
        twin.step_tensor(shifted.contiguous(), ref[0], ref[1], ref[2], terminal_obs=ref[3])
        torch.cuda.synchronize()
        fin = ref[2].bool()
        for g, r in zip(got[:3], ref[:3]):
            assert np.array_equal(_bits(g) if g.dtype == torch.float32 else g.cpu().numpy(), _bits(r) if r.dtype == torch.float32 else r.cpu().numpy()), k
        assert np.array_equal(_bits(got[3])[fin.cpu().numpy()], _bits(ref[3])[fin.cpu().numpy()])
        first = fin
        finished += int(fin.sum())
    assert finished >= n                                     # every env went through an auto-reset
    snap = env.snapshot()
    env.restore(snap)
    assert np.array_equal(env.perturbation.state()["age"], snap["perturbation"]["age"])
    env.close(), twin.close()


@pytest.mark.parametrize("kind", ["po", "plain"])
def test_numpy_cold_path_gives_the_device_paths_rows(kind):
    """reset() / step() on host arrays run the same two launches: with noise, bias and latency on, their observations and terminal
    observations are the bits step_tensor leaves (a finished env's row: its reset stack for the PO env, zeros beside the terminal
    observation in infos for the plain one)."""
    from quadruped_gym_amd.envs.vec_env import QuadrupedVecEnv
    n, steps = 8, 12
    if kind == "po":
        inner, twin = _po_envs()
        noise = {"gyro": 0.01, "accel": 0.02, "euler": 0.005, "body_vel": 0.01}
    else:
        kw = dict(reward_fns={"forward": 1.0, "control_cost": -0.1, "alive_bonus": 1.0}, termination_fns={"fall": 0.05}, max_time=0.04)
        inner, twin = QuadrupedVecEnv(n, **kw), QuadrupedVecEnv(n, **kw)
        noise = {"accel": 0.02, "gyro": 0.01, "body_vel": 0.01}
    opts = dict(obs_noise=noise, obs_bias={"gyro": 0.02}, action_noise=0.02, action_latency=(0.0, 0.016), seed=9)
    host, dev = DevicePerturbedVecEnv(inner, **opts), DevicePerturbedVecEnv(twin, **opts)
    D = inner.obs_dim
    first = host.reset()
    assert np.array_equal(first.view(np.uint32), dev.reset().view(np.uint32)) and (kind == "plain" or np.abs(first).max() > 0)
    assert host.perturbation.delays().max() > 0 and np.array_equal(host.perturbation.delays(), dev.perturbation.delays())
    acts = np.random.default_rng(4).uniform(-1, 1, (steps, n, 12)).astype(np.float32)
    mk = lambda *s, dt=torch.float32: torch.zeros(s, device=DEV, dtype=dt)     # noqa: E731
    finished = 0
    for k in range(steps):
        obs, rew, done, infos = host.step(acts[k])
        if kind == "po":
            t_obs, t_rew, t_done, t_term = mk(n, D), mk(n), mk(n, dt=torch.uint8), mk(n, D)
            dev.step_tensor(_t(acts[k]), t_obs, t_rew, t_done, terminal_obs=t_term)
            want_obs, want_done, want_term = t_obs.cpu().numpy(), t_done.cpu().numpy().astype(bool), t_term.cpu().numpy()
        else:
            packed = dev.step_tensor(_t(acts[k])).cpu().numpy()
            want_done = packed[:, D + 1] != 0
            want_term = packed[:, :D]
            want_obs = np.where(want_done[:, None], np.float32(0.0), packed[:, :D])
        assert np.array_equal(np.asarray(done, bool), want_done), k
        assert np.array_equal(np.ascontiguousarray(obs, dtype=np.float32).view(np.uint32), np.ascontiguousarray(want_obs).view(np.uint32)), k
        for i in np.nonzero(want_done)[0]:
            got = np.asarray(infos[int(i)]["terminal_observation"], np.float32)
            assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want_term[i]).view(np.uint32)), (k, i)
        finished += int(want_done.sum())
    assert finished >= n
    hs, ds = host.perturbation.state(), dev.perturbation.state()
    assert all(np.array_equal(hs[key].view(np.uint8), ds[key].view(np.uint8)) for key in ("age", "episode", "ring"))
    host.close(), dev.close()


def test_plain_env_packed_rows_through_the_wrapper():
    from quadruped_gym_amd.envs.vec_env import QuadrupedVecEnv
    kw = dict(reward_fns={"forward": 1.0, "control_cost": -0.1, "alive_bonus": 1.0}, termination_fns={"fall": 0.05}, max_time=0.04)
    inner, twin = QuadrupedVecEnv(8, **kw), QuadrupedVecEnv(8, **kw)
    env = DevicePerturbedVecEnv(inner, seed=3)
    assert env.perturbation.done_row == "terminal" and (env.perturbation.frame_dim, env.perturbation.window) == (33, 1)
    assert np.array_equal(env.reset(), twin.reset())
    gen = torch.Generator(device=DEV)
    gen.manual_seed(6)
    acts = torch.rand((8, 8, 12), generator=gen, device=DEV) * 2 - 1
    dones = 0
    for k in range(8):
        got, ref = env.step_tensor(acts[k]), twin.step_tensor(acts[k])
        torch.cuda.synchronize()
        assert np.array_equal(_bits(got), _bits(ref)), k
        dones += int(ref[:, 34].sum())
    st = env.perturbation.state()
    assert dones >= 8 and int(st["episode"].sum()) == dones + 8      # reset() began episode 1 everywhere
    # and with noise on the sensor groups only those columns move
    noisy = DevicePerturbedVecEnv(twin, obs_noise={"accel": 0.01, "gyro": 0.01, "body_vel": 0.01}, seed=3)
    a = acts[0].clone()
    got = noisy.step_tensor(a).clone()
    raw = inner.step_tensor(acts[0])
    torch.cuda.synchronize()
    moved = (_bits(got) != _bits(raw)).any(0)
    assert torch.equal(a, acts[0]) and moved[12:18].all() and moved[30:33].all() and not moved[:12].any() and not moved[18:30].any()
    assert not moved[33:].any() and float((got - raw).abs().max()) < 0.01 * 5.78
    env.perturbation.close(), noisy.perturbation.close()
    inner.close(), twin.close()
