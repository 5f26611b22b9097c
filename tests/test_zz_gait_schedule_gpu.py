"""The gait schedule on the GPU (qg_sched_*, csrc/qg_sched.hip) against tests/gait_schedule_reference.py: phase, episode, gait row,
frequency, d, contact_match, the zeros of finished envs and passed-through rewards EXACTLY; the three float terms, the components, the
shaped reward and the sin / cos columns against the float64 definition -- evaluated on the sensor's own non-advancing read of the same
state, so every flag of the reference is exact -- within MARGIN x the CPU-measured float32 budget.  Then the scripted done table with
both done_row meanings, the sensor left untouched, shards, strides, graph replay, the wrapper and the refusals.
The module's name puts it last in collection, as the other modules that capture hipGraphs on a side stream."""
import numpy as np
import pytest
import torch

import contact_cells as CC
import gait_reward_reference as G
import gait_schedule_reference as R

from quadruped_gym_amd import _abi
from quadruped_gym_amd.contact import ContactSensor
from quadruped_gym_amd.gait import DeviceGaitRewardVecEnv, GaitReward
from quadruped_gym_amd.schedule import DeviceGaitScheduleVecEnv, GaitSchedule
from quadruped_gym_amd.sim import BatchedSim

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OPTS = dict(R.LIMITS, random_phase=True)
BLOB_HEADER = 24                                           # the snapshot blob: header, phi [n] u32, episode [n] i64


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


def _bits(*tensors):
    torch.cuda.synchronize()
    return np.concatenate([t.detach().cpu().contiguous().numpy().astype(np.float32).view(np.uint32).ravel() for t in tensors])


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _task(frame_skip=R.FRAME_SKIP, walk=False):
    t = G.walk_task(_abi) if walk else _abi.default_task()
    t.frame_skip = frame_skip
    return t


@pytest.fixture(scope="module")
def fix():
    f = CC.load()
    f["idx"] = R.fixture_states(f)
    return f


def _loaded(fix, sel=slice(None), seed=0, done_row="terminal", base=0, **kw):
    """(sim, sensor, schedule) holding the fixture states idx[sel], dt = 0.02 s."""
    idx = fix["idx"][sel]
    sim = BatchedSim(len(idx), task=_task())
    sim.set_state(fix["qpos"][idx], fix["qvel"][idx], fix["act"][idx], None, fix["nstep"][idx])
    sensor = ContactSensor(sim, R.FORCE_THRESHOLD)
    sched = GaitSchedule(sensor, R.TABLE, R.FREQ, R.WEIGHTS, done_row=done_row, seed=seed, env_index_base=base, **dict(OPTS, **kw))
    return sim, sensor, sched


def _close(*handles):
    for h in handles:
        h.close()


def _state(sched):
    blob, n = sched.state(), sched.num_envs
    return blob[BLOB_HEADER:BLOB_HEADER + 4 * n].view(np.uint32).copy(), blob[BLOB_HEADER + 4 * n:].view(np.int64).copy()


def _check_ints(sched, chk):
    """phi, episode, gait row and freq of the handle equal the checker's, exactly."""
    got, want = sched.gaits(), chk.gaits()
    phi, episode = _state(sched)
    assert np.array_equal(phi, want["phi"].astype(np.uint32)) and np.array_equal(got["phi"], phi)
    assert np.array_equal(episode, chk.episode) and np.array_equal(got["gait"], want["gait"])
    assert _same(got["freq"], want["freq"])


_check_columns = R.check_columns                           # shared with tests/test_zz_wrapper_stacks_gpu.py


def _check_terms(what, view, comps, reward_out, force, feet, done=None, command=None, reward=None, kappa=R.KAPPA, weights=R.WEIGHTS):
    """components [n, 4] and reward_out against the float64 definition on (force, feet): MARGIN x the budget; contact_match equal."""
    ref = R.evaluate(view, force, feet, done, command, reward, **dict(R.PARAMS, kappa=kappa, weights=weights))
    tol_c, tol_r = R.component_tolerance(ref, weights, R.MARGIN), R.reward_tolerance(ref, weights, reward, R.MARGIN)
    err_c, err_r = np.abs(comps.astype(np.float64) - ref["components"]), np.abs(reward_out.astype(np.float64) - ref["reward_out"])
    assert (err_c <= tol_c).all() and (err_r <= tol_r).all(), (what, err_c.max(0), err_r.max())
    assert np.array_equal(comps[:, 3].astype(np.float64), ref["components"][:, 3]), what            # contact_match: exact
    finished = np.zeros(len(comps), bool) if done is None else np.asarray(done) != 0
    assert not comps[finished].any()
    if reward is not None:
        assert _same(reward_out[finished], np.asarray(reward, np.float32)[finished])
    ok = tol_c > 0
    return ref, (float((err_c[ok] / tol_c[ok]).max()) if ok.any() else 0.0), float((err_r / np.where(tol_r > 0, tol_r, 1.0)).max())


# ---- 1. the fixture states ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
def test_fixture_terms_and_columns_are_the_reference(fix, n):
    sim, sensor, sched = _loaded(fix, slice(0, n))
    chk = R.Checker(n, seed=0, **R.PARAMS)
    _check_ints(sched, chk)                                                         # a new handle: episode 0 at its phi0
    done, command, reward, base = (a[:n] for a in R.extras(67))
    force, feet = (t.cpu().numpy() for t in sensor.read(advance=False))
    obs = R.obs_rows(n, 33, 1)[0]
    d_obs, d_cmd, d_rew, d_base, d_done = _dev(obs), _dev(command), _dev(reward), _dev(base), _dev(done, np.uint8)
    worst, cells = [0.0, 0.0, 0.0], set()
    for t in range(R.STEPS):
        fin = done if t % 8 == 5 else None
        wide, out, rows = sched.step(d_done if fin is not None else None, d_rew, base_components=d_base, command=d_cmd, obs=d_obs)
        row, old = chk.step(fin)
        wide, out, rows = (x.cpu().numpy() for x in (wide, out, rows))
        ref, sc, sr = _check_terms("step %d" % t, old, wide[:, R.C0:], out, force, feet, fin, command, reward)
        assert _same(wide[:, :R.C0], base) and _same(rows[:, :33], obs)             # copied in front: the bits
        worst = [max(a, b) for a, b in zip(worst, (sc, sr, _check_columns("step %d" % t, rows[:, 33:], row)))]
        cells |= {(f, bool(h), bool(c)) for f in range(4) for h, c in zip(ref["hard"][:, f], ref["contact"][:, f])}
    _check_ints(sched, chk)
    print("n = %d: components' largest share of the bound %.3f, reward %.3f; clock columns' largest |gpu - f64| %.3e (bound %.1e)"
          % (n, worst[0], worst[1], worst[2], R.MARGIN * R.BUDGET_CLOCK))
    if n == 67:
        assert len(cells) == 16                                                     # every foot in each of the four cells
    _close(sched, sensor, sim)


def test_kappa_zero_is_the_hard_schedule(fix):
    sim, sensor, sched = _loaded(fix, kappa=0.0)
    chk = R.Checker(67, seed=0, **R.PARAMS)
    force, feet = (t.cpu().numpy() for t in sensor.read(advance=False))
    for t in range(5):
        comps, out, _ = sched.step()
        _, old = chk.step()
        _check_terms("step %d" % t, old, comps.cpu().numpy(), out.cpu().numpy(), force, feet, kappa=0.0)
    _close(sched, sensor, sim)


# ---- 2. a walk: the integers at every step, through wraps and auto-resets ----------------------------------------------------------------
class _Run:
    """The gait tests' walk recipe at dt = 0.02 s (10 env-steps per episode) with the schedule's launch behind every env-step."""

    def __init__(self, seed=1):
        n = G.N_WALK
        self.sim = BatchedSim(n, task=_task(walk=True))
        self.sim.reset(seed=G.WALK_RESET_SEED)
        self.sensor = ContactSensor(self.sim, R.FORCE_THRESHOLD)
        self.sched = GaitSchedule(self.sensor, R.TABLE, R.FREQ, R.WEIGHTS, seed=seed, **OPTS)
        self.packed = torch.zeros((n, 35), device=DEV)
        self.comps, self.out, self.rows = torch.zeros((n, 4), device=DEV), torch.zeros(n, device=DEV), torch.zeros((n, 43), device=DEV)

    def step(self, actions, stream=None):
        self.sim.step_device_packed(actions, self.packed, stream=stream)
        self.sched.step(self.packed[:, 34], self.packed[:, 33], self.out, self.comps, obs=self.packed[:, :33], out=self.rows, stream=stream)

    def bits(self):
        return _bits(self.packed, self.comps, self.out, self.rows)

    def close(self):
        _close(self.sched, self.sensor, self.sim)


@pytest.fixture(scope="module")
def walk():
    """The eager run: per step the output bits, the done vector and the handle's integers."""
    run, acts = _Run(), _dev(G.walk_actions())
    bits, dones, ints = [], [], []
    for t in range(R.STEPS):
        run.step(acts[t])
        bits.append(run.bits())
        dones.append(run.packed[:, 34].cpu().numpy() != 0)
        ints.append((run.sched.gaits(), _state(run.sched)))
    run.close()
    return dict(bits=bits, dones=dones, ints=ints)


def test_walk_integers_are_the_reference_at_every_step(walk):
    chk = R.Checker(G.N_WALK, seed=1, **R.PARAMS)
    wraps, resets, gaits_seen = 0, 0, set()
    for t in range(R.STEPS):
        before = chk.phi.copy()
        chk.step(walk["dones"][t])
        got, (phi, episode) = walk["ints"][t]
        want = chk.gaits()
        assert np.array_equal(phi, want["phi"].astype(np.uint32)) and np.array_equal(episode, chk.episode), t
        assert np.array_equal(got["gait"], want["gait"]) and _same(got["freq"], want["freq"]) and np.array_equal(got["phi"], phi), t
        live = ~walk["dones"][t]
        wraps += int((chk.phi[live] < before[live]).sum())
        resets += int(walk["dones"][t].sum())
        gaits_seen |= set(want["gait"].tolist())
    print("%d wraps, %d auto-resets, gait rows seen %s" % (wraps, resets, sorted(gaits_seen)))
    assert wraps >= 67 and resets >= 3 * 67 and gaits_seen == set(range(len(R.TABLE))) and chk.episode.min() >= 3


# ---- 3. the scripted done table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("done_row,kind", [("terminal", "u8"), ("terminal", "f32"), ("reset", "u8"), ("reset", "f32")])
def test_scripted_done_table(fix, n, done_row, kind):
    sim, sensor, sched = _loaded(fix, slice(0, n), seed=12345, done_row=done_row)
    chk = R.Checker(n, seed=12345, done_row=done_row, **R.PARAMS)
    table, obs, term = R.done_table(n), R.obs_rows(n, 33, tag=1), R.obs_rows(n, 33, tag=2)
    force, feet = (t.cpu().numpy() for t in sensor.read(advance=False))
    reward = R.extras(67)[2][:n]
    d_rew, mark = _dev(reward), 4321.0
    strided = torch.zeros((n, 3), device=DEV)                                       # a float32 done vector at stride 3
    new_gait = 0
    for t in range(R.STEPS):
        fin = table[t] != 0
        if kind == "u8":
            d_done = _dev(table[t])
        else:
            strided[:, 1] = _dev(table[t].astype(np.float32))
            d_done = strided[:, 1]
        t_out = torch.full((n, 43), mark, device=DEV) if done_row == "reset" else None
        g_before = chk.gaits()["gait"]
        comps, out, rows = sched.step(d_done, d_rew, obs=_dev(obs[t]), terminal_obs=_dev(term[t]) if t_out is not None else None,
                                      terminal_out=t_out)
        row, old = chk.step(fin)
        comps, out, rows = (x.cpu().numpy() for x in (comps, out, rows))
        _check_terms("step %d" % t, old, comps, out, force, feet, fin, None, reward)
        _check_columns("step %d rows" % t, rows[:, 33:], row)
        assert _same(rows[:, :33], obs[t])
        if done_row == "reset" and fin.any():                                       # the row shows the NEW episode at its phi0
            g1, fr1, phi1 = chk.draw(chk.episode)
            assert np.array_equal(row["phi"][fin], phi1[fin]) and _same(rows[fin, 41], fr1[fin])
        if t_out is not None:
            t_out = t_out.cpu().numpy()
            assert (t_out[~fin] == mark).all()                                      # rows of live envs: not touched
            if fin.any():
                assert _same(t_out[fin, :33], term[t][fin])
                _check_columns("step %d terminal rows" % t, t_out[fin, 33:], {k: v[fin] for k, v in old.items()})
        new_gait += int((chk.gaits()["gait"][fin] != g_before[fin]).sum())
        _check_ints(sched, chk)
    assert chk.episode.max() == (4 if n >= 5 else 0) and (n < 5 or new_gait >= 1)    # a new gait was drawn for a new episode
    # begin: a masked explicit reset writes the new episode's columns, and only those rows
    mask = np.arange(n) % 2 == 0
    rows = torch.full((n, 45), mark, device=DEV)
    sched.begin(_dev(mask, np.uint8), rows, obs_dim=33)
    view, sel = chk.begin(mask)
    rows = rows.cpu().numpy()
    _check_ints(sched, chk)
    _check_columns("begin", rows[sel, 33:43], {k: v[sel] for k, v in view.items()})
    assert (rows[:, :33] == mark).all() and (rows[:, 43:] == mark).all() and (rows[~sel] == mark).all()
    sched.begin()
    chk.begin()
    _check_ints(sched, chk)
    _close(sched, sensor, sim)


# ---- 4. the sensor is left alone -----------------------------------------------------------------------------------------------------------
def test_sensor_state_is_untouched_and_the_gait_reward_composes(fix):
    sim, sensor, sched = _loaded(fix)
    gait = GaitReward(sensor, G.WEIGHTS, **{k: v for k, v in G.PARAMS.items() if k != "weights"})
    sensor.read(advance=True)                                                       # armed, one step into a phase
    before, s0 = sensor.state(), sched.state()
    comps, out, _ = sched.step()
    torch.cuda.synchronize()
    assert np.array_equal(sensor.state(), before)                                   # byte-identical: timers and armed flags
    force, feet = sensor.read(advance=False)
    assert np.array_equal(sensor.state(), before)
    chk = R.Checker(67, seed=0, **R.PARAMS)
    hard = R.foot_quantities(chk.step()[1]["phi"], chk.gaits()["gait"])[0]
    contact = feet[..., 6].cpu().numpy() > 0.5
    assert np.array_equal(comps[:, 3].cpu().numpy(), np.float32(R.WEIGHTS["contact_match"]) * (contact == hard).sum(1).astype(np.float32))
    # the gait reward's advancing launch before or after the schedule's: no bit of either's outputs changes
    results = []
    for first in ("schedule", "gait"):
        sensor.load_state(before), sched.load_state(s0)
        if first == "schedule":
            a = sched.step()
            b = gait.step()
        else:
            b = gait.step()
            a = sched.step()
        results.append((_bits(a[0], a[1]), _bits(b[0], b[1]), sensor.state().copy(), sched.state().copy()))
    for x, y in zip(*results):
        assert np.array_equal(x, y)
    assert not np.array_equal(results[0][2], before)                                # (the gait launch did advance the timers)
    _close(gait, sched, sensor, sim)


# ---- 5. shards -----------------------------------------------------------------------------------------------------------------------------
def test_shards_with_env_index_base_reproduce_the_handle(fix):
    table, obs = R.done_table(67), R.obs_rows(67, 33, tag=3)
    reward = R.extras(67)[2]

    def run(lo, hi):
        sim, sensor, sched = _loaded(fix, slice(lo, hi), seed=1, done_row="reset", base=1000 + lo)
        bits = []
        for t in range(12):
            t_out = torch.zeros((hi - lo, 43), device=DEV)
            comps, out, rows = sched.step(_dev(table[t][lo:hi]), _dev(reward[lo:hi]), obs=_dev(obs[t][lo:hi]), terminal_obs=_dev(obs[t][lo:hi]),
                                          terminal_out=t_out)
            bits.append([x.cpu().numpy() for x in (comps, out, rows, t_out)])
        ints = sched.gaits()
        _close(sched, sensor, sim)
        return bits, ints

    whole, ints = run(0, 67)
    for lo, hi in ((0, 1), (1, 6), (6, 67)):
        part, p_ints = run(lo, hi)
        for t in range(12):
            for a, b in zip(part[t], whole[t]):
                assert _same(a, b[lo:hi]), (lo, hi, t)
        assert all(np.array_equal(p_ints[k], ints[k][lo:hi]) for k in ints)


# ---- 6. strides and outputs ----------------------------------------------------------------------------------------------------------------
def test_strided_in_place_and_omitted_outputs(fix):
    n, mark = 67, 12345.0
    done, command, reward, base = R.extras(n)
    obs = R.obs_rows(n, 33, 1)[0]
    sim, sensor, sched = _loaded(fix)
    s0 = sched.state()
    want_wide, want_out, want_rows = (x.cpu().numpy() for x in sched.step(_dev(done, np.uint8), _dev(reward), base_components=_dev(base),
                                                                          command=_dev(command), obs=_dev(obs)))
    s1 = sched.state()
    # everything a column slice of a wider buffer; the reward in place; an odd-width observation (element copies)
    sched.load_state(s0)
    buf, base_buf = torch.full((n, 20), mark, device=DEV), torch.full((n, 13), mark, device=DEV)
    base_buf[:, 1:12] = _dev(base)
    packed, frame = torch.full((n, 36), mark, device=DEV), torch.full((n, 47), mark, device=DEV)
    packed[:, 1:34], packed[:, 34], packed[:, 35] = _dev(obs), _dev(reward), _dev(done, np.float32)
    cmd = torch.full((n, 5), mark, device=DEV)
    cmd[:, 2:4] = _dev(command)
    comps, out, rows = sched.step(packed[:, 35], packed[:, 34], packed[:, 34], buf[:, 2:17], base_buf[:, 1:12], cmd[:, 2:4], packed[:, 1:34],
                                  frame[:, 3:46])
    assert comps.data_ptr() == buf[:, 2:17].data_ptr() and out.data_ptr() == packed[:, 34].data_ptr()
    assert _same(buf[:, 2:17].cpu().numpy(), want_wide) and _same(packed[:, 34].cpu().numpy(), want_out)
    assert _same(frame[:, 3:46].cpu().numpy(), want_rows) and np.array_equal(sched.state(), s1)
    for t, cols in ((buf, [0, 1, 17, 18, 19]), (packed, [0]), (base_buf, [0, 12]), (frame, [0, 1, 2, 46]), (cmd, [0, 1, 4])):
        assert (t[:, cols] == mark).all()                                           # the bytes outside: untouched
    # the observation already in place (obs == out at the same stride): only the ten columns are written; base columns in place too
    sched.load_state(s0)
    own, wide = torch.full((n, 48), mark, device=DEV), torch.full((n, 16), mark, device=DEV)
    own[:, :33], wide[:, :R.C0] = _dev(obs), _dev(base)
    sched.step(_dev(done), _dev(reward), components=wide[:, :15], base_components=wide[:, :R.C0], command=_dev(command), obs=own[:, :33],
               out=own[:, :43])
    assert _same(own[:, :43].cpu().numpy(), want_rows) and (own[:, 43:] == mark).all()
    assert _same(wide[:, :15].cpu().numpy(), want_wide) and (wide[:, 15] == mark).all()
    # omitted outputs: no rows; the ten columns alone; a 16-byte-aligned width takes the vector copy: the same bits
    sched.load_state(s0)
    comps, out, rows = sched.step(_dev(done, np.uint8), _dev(reward), command=_dev(command))
    assert rows is None and _same(comps.cpu().numpy(), want_wide[:, R.C0:]) and _same(out.cpu().numpy(), want_out)
    sched.load_state(s0)
    comps, out, _ = sched.step(_dev(done, np.uint8), command=_dev(command))           # no reward: the shaped sum alone
    ref_shaped = want_wide[:, R.C0:].astype(np.float32)
    acc = ref_shaped[:, 0].copy()
    for k in range(1, 4):
        acc = (acc + ref_shaped[:, k]).astype(np.float32)
    assert _same(out.cpu().numpy(), acc)
    sched.load_state(s0)
    only = torch.full((n, 12), mark, device=DEV)
    sched.step(_dev(done, np.uint8), out=only[:, 1:11])
    assert _same(only[:, 1:11].cpu().numpy(), want_rows[:, 33:]) and (only[:, [0, 11]] == mark).all()
    sched.load_state(s0)
    obs32 = R.obs_rows(n, 32, 1, tag=5)[0]
    a32 = torch.full((n, 44), mark, device=DEV)
    sched.step(_dev(done, np.uint8), obs=_dev(obs32), out=a32[:, :42])                # aligned rows at stride 44: float4 copies
    assert _same(a32[:, :32].cpu().numpy(), obs32) and _same(a32[:, 32:42].cpu().numpy(), want_rows[:, 33:]) and (a32[:, 42:] == mark).all()
    _close(sched, sensor, sim)


# ---- 7. graph replay -----------------------------------------------------------------------------------------------------------------------
def test_graph_replay_is_the_eager_run(walk):
    """One env-step and the schedule's launch behind it, captured once and replayed 20 times: the bits of 20 eager steps -- the phase
    and the episode advance on the device under replay."""
    run, acts = _Run(), _dev(G.walk_actions())
    fresh, sim0 = run.sched.state(), run.sim.snapshot()
    s_act = torch.zeros((G.N_WALK, 12), device=DEV)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run.step(s_act, stream=side)
    run.sim.restore(sim0)                                                          # whatever a capture may have run, start from the fresh state
    run.sched.load_state(fresh)
    for t in range(20):
        s_act.copy_(acts[t])
        torch.cuda.synchronize()
        graph.replay()
        assert np.array_equal(run.bits(), walk["bits"][t]), t
    del graph
    run.close()


# ---- 8. set_weights ------------------------------------------------------------------------------------------------------------------------
def test_set_weights_applies_to_the_next_launch(fix):
    sim, sensor, sched = _loaded(fix)
    s0 = sched.state()
    a, _, _ = sched.step()
    sched.load_state(s0)
    sched.set_weights({"contact_match": 0.25, "swing_height": 0.0})
    b, _, _ = sched.step()
    torch.cuda.synchronize()
    assert torch.equal(b[:, 3], 2 * a[:, 3]) and not b[:, 2].any() and torch.equal(a[:, :2], b[:, :2]) and a[:, 2].any() and a[:, 3].any()
    assert sched.weights["contact_match"] == 0.25 and sched.weights["swing_force"] == R.WEIGHTS["swing_force"]
    with pytest.raises(ValueError):
        sched.set_weights({"nope": 1.0})
    _close(sched, sensor, sim)


# ---- 9. the wrapper ------------------------------------------------------------------------------------------------------------------------
WALK = dict(max_time=0.1, device_commands=True, random_controls=True, nan_direction=False)
GAIT_KW = dict(weights=G.WEIGHTS, force_threshold=R.FORCE_THRESHOLD, **{k: v for k, v in G.PARAMS.items() if k != "weights"})
SCHED_KW = dict(gaits=R.TABLE, freq=R.FREQ, weights=R.WEIGHTS, force_threshold=R.FORCE_THRESHOLD, seed=7, **OPTS)


def test_wrapper_snapshot_continues_bit_for_bit():
    from quadruped_gym_amd.envs.walking import WalkingQuadrupedVecEnv
    n = 33
    acts = _dev(np.random.default_rng(5).uniform(-1, 1, (30, n, 12)).astype(np.float32))

    def make():
        env = DeviceGaitScheduleVecEnv(WalkingQuadrupedVecEnv(n, **WALK), **SCHED_KW)
        first = env.reset()
        return env, first, [torch.zeros(s, device=DEV) for s in ((n, 43), (n,))] + [torch.zeros(n, device=DEV, dtype=torch.uint8),
                                                                                    torch.zeros((n, 15), device=DEV)]

    def run(env, bufs, lo, hi):
        out = []
        for t in range(lo, hi):
            env.step_tensor(acts[t], *bufs)
            out.append(_bits(bufs[0], bufs[1], bufs[3]))
        return out

    env, first, bufs = make()
    assert env.obs_dim == 43 and env.observation_space.shape == (43,) and first.shape == (n, 43) and env.schedule.done_row == "terminal"
    chk = R.Checker(n, seed=7, **R.PARAMS)
    view, _ = chk.begin()                                                           # reset() began episode 1
    _check_columns("reset", first[:, 33:], view)
    run(env, bufs, 0, 12)
    snap = env.snapshot()
    assert snap["gait_schedule"].dtype == np.uint8 and "contact" in snap["env"]
    want = run(env, bufs, 12, 30)
    env2, _, bufs2 = make()
    env2.restore(snap)
    got = run(env2, bufs2, 12, 30)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert bufs[3][:, 11:].any()                                                    # the schedule's columns are paid
    # the NumPy cold path: wide rows, shaped rewards, the four columns beside them, wide terminal observations
    finished = 0
    for _ in range(12):                                                             # through the episode end at env-step 39
        obs, rew, dones, infos = env2.step(np.zeros((n, 12), np.float32))
        assert obs.shape == (n, 43) and rew.shape == (n,) and env2.last_schedule_components.shape == (n, 4) and len(infos) == n
        for i in np.flatnonzero(dones):
            assert infos[i]["terminal_observation"].shape == (43,)
            finished += 1
        now = env2.schedule.gaits()
        assert _same(obs[:, 41], now["freq"])                                       # every row shows its running episode's frequency
    assert finished >= n
    sensor, sched = env.venv._contact, env.schedule
    env.close(), env2.close()
    assert sensor._h is None and sched._h is None                                   # closed with the env, the layer first


def test_stacks_with_the_other_device_wrappers():
    """Normaliser(privileged(schedule(gait(perturbation(partially observable env))))) against the layers' calls made by hand around a
    twin env: the same wide rows, rewards and 22 component columns, bit for bit, through episode ends."""
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
    from quadruped_gym_amd.monitor import RewardMonitor
    from quadruped_gym_amd.normalize import DeviceVecNormalize
    from quadruped_gym_amd.perturb import DevicePerturbedVecEnv
    from quadruped_gym_amd.policy import FusedMlpPolicy
    from quadruped_gym_amd.privileged import DevicePrivilegedVecEnv
    n, T, window = 67, 25, 3
    O = 26 * window

    def inner():
        base = POWalkingQuadrupedVecEnv(n, obs_window=window, reset_options={"min_speed": 0.0, "max_speed": 0.3}, **WALK)
        return DeviceGaitRewardVecEnv(DevicePerturbedVecEnv(base, obs_noise={"gyro": 0.01}, seed=1), gate_on_command=True, **GAIT_KW)

    sched_env = DeviceGaitScheduleVecEnv(inner(), gate_on_command=True, **SCHED_KW)
    env = DeviceVecNormalize(DevicePrivilegedVecEnv(sched_env, R.FORCE_THRESHOLD), norm_obs=False, norm_reward=False)
    assert sched_env.schedule.done_row == "reset" and sched_env.obs_dim == O + 10 and env.obs_dim == O + 10 + 85
    assert env.reward_keys == list(sched_env.venv.venv.venv.reward_keys) + list(G.TERMS) + list(R.TERMS) and len(env.reward_keys) == 22
    mon = RewardMonitor.for_env(env, capacity=T)
    assert mon.n_terms == 22
    twin = inner()
    hand = GaitSchedule(twin.contact_sensor(R.FORCE_THRESHOLD), R.TABLE, R.FREQ, R.WEIGHTS, done_row="reset", seed=7,
                        env_index_base=0, **OPTS)
    pack = twin.privileged_state(R.FORCE_THRESHOLD)
    env.reset(), twin.reset(), hand.begin()
    z = lambda *s, **kw: torch.zeros(s, device=DEV, **kw)
    obs, rew, done, comps, term = z(n, O + 95), z(n), z(n, dtype=torch.uint8), z(n, 22), z(n, O + 10)
    t_obs, t_rew, t_done, t_comps, t_term = z(n, O), z(n), z(n, dtype=torch.uint8), z(n, 18), z(n, O)
    h_comps, h_rows, h_term, h_wide = z(n, 22), z(n, O + 10), z(n, O + 10), z(n, O + 95)
    policy = FusedMlpPolicy(sched_env.obs_dim, (32, 32), 12, critic_obs=(0, O + 95))
    policy.set_params(np.random.default_rng(8).normal(0, 0.1, policy.n_params).astype(np.float32))
    acts = _dev(np.random.default_rng(6).uniform(-1, 1, (T, n, 12)).astype(np.float32))
    ends = 0
    for t in range(T):
        env.step_tensor(acts[t], obs, rew, done, components=comps, terminal_obs=term)
        mon.record(comps, rew, done)
        twin.step_tensor(acts[t], t_obs, t_rew, t_done, components=t_comps, terminal_obs=t_term)
        lo = 26 * (window - 1) + 23
        hand.step(t_done, t_rew, t_rew, h_comps, t_comps, t_obs[:, lo:lo + 2], t_obs, h_rows, t_term, h_term)
        pack.read(h_wide, h_rows)
        assert np.array_equal(_bits(obs, rew, comps), _bits(h_wide, t_rew, h_comps)), t
        fin = done.cpu().numpy() != 0
        assert np.array_equal(_bits(term[_dev(fin)]), _bits(h_term[_dev(fin)])), t
        ends += int(fin.sum())
    assert ends >= n and torch.isfinite(obs).all()
    rows = mon.rows()
    assert all(np.isfinite(rows[k]).all() for k in mon.keys) and len(rows["reward"]) == T and any(rows[k].any() for k in R.TERMS)
    # a policy's forward pass on the wide row: the actor reads [0 : O + 10], clock included; the critic the whole row
    a_out, value = z(n, 12), z(n)
    policy.forward(obs, a_out, value=value)
    torch.cuda.synchronize()
    assert torch.isfinite(a_out).all() and torch.isfinite(value).all() and a_out.any()
    _close(policy, mon, hand)
    env.close(), twin.close()


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch(fix):
    n = 5
    sim, sensor, sched = _loaded(fix, slice(0, n), done_row="reset")
    before, s_before = sensor.state(), sched.state()
    z = lambda *shape, **kw: torch.zeros(shape, device=DEV, **kw)
    wide = z(n, 64)
    bad = [dict(reward=z(n).double()), dict(reward=z(n + 1)), dict(reward_out=z(n, 2)), dict(reward_out=z(n).cpu()), dict(components=z(n, 5)),
           dict(components=z(4, n).t()), dict(components=z(n, 4), base_components=z(n, 3)), dict(base_components=z(n, 29)),
           dict(base_components=z(n, 11).double()), dict(command=z(n, 3)), dict(command=z(2, n).t()), dict(done=z(n, dtype=torch.int32)),
           dict(done=z(n - 1)), dict(obs=z(n, 33), out=z(n, 42)), dict(obs=z(n, 33).half()), dict(out=z(n, 11)), dict(obs=z(33, n).t()),
           dict(terminal_obs=z(n, 33)), dict(obs=z(n, 33), terminal_obs=z(n, 32), terminal_out=z(n, 42)),
           dict(obs=z(n, 33), terminal_out=z(n, 43)),
           # overlapping rows: the observation behind the front of the wide rows, or the same columns at another stride
           dict(obs=wide[:, 4:37], out=wide[:, :43]), dict(obs=wide[:, :33], out=wide[:, 1:44]),
           dict(components=wide[:, :15], base_components=wide[:, 4:15]), dict(components=wide[:, 2:17], base_components=wide[:, :11])]
    for kw in bad:
        with pytest.raises(ValueError):
            sched.step(**kw)
    for kw in (dict(mask=z(n)), dict(mask=z(2 * n, dtype=torch.uint8)[::2]), dict(rows=z(n, 9)), dict(rows=z(n, 43), obs_dim=34)):
        with pytest.raises(ValueError):
            sched.begin(**kw)
    lib = _abi.load_library()
    ptr = wide.data_ptr()
    names = (("h", sched._h), ("done", None), ("kind", 0), ("dstride", 1), ("reward", None), ("rstride", 1), ("out_r", ptr), ("ostride", 1),
             ("comps", None), ("cstride", 4), ("base", None), ("bstride", 0), ("c0", 0), ("cmd", None), ("mstride", 2), ("obs", None),
             ("obs_stride", 0), ("obs_dim", 0), ("out", None), ("out_stride", 0), ("t_obs", None), ("t_obs_stride", 0), ("t_out", None),
             ("t_out_stride", 0), ("stream", None))
    args = lambda **kw: [kw.get(k, v) for k, v in names]
    for kw, word in ((dict(ostride=0), b"reward_out_stride"), (dict(reward=ptr, rstride=0), b"reward_stride"),
                     (dict(reward=ptr, out_r=None), b"reward without reward_out"), (dict(comps=ptr, cstride=3), b"components_stride"),
                     (dict(comps=ptr, cstride=40, base=ptr + 4096, bstride=29, c0=29), b"base_terms"), (dict(c0=3), b"without base_components"),
                     (dict(base=ptr, c0=2, bstride=2), b"without components"),
                     (dict(comps=ptr, cstride=20, base=ptr + 16, bstride=20, c0=11), b"overlap"), (dict(cmd=ptr, mstride=1), b"command_stride"),
                     (dict(done=ptr, kind=2), b"done_kind"), (dict(done=ptr, dstride=0), b"done_stride"), (dict(obs_dim=-1), b"obs_dim"),
                     (dict(out=ptr, out_stride=42, obs_dim=33, obs=ptr + 8192, obs_stride=33), b"out_stride"),
                     (dict(out=ptr, out_stride=43, obs_dim=33), b"without obs"),
                     (dict(out=ptr, out_stride=43, obs_dim=33, obs=ptr + 4, obs_stride=43), b"overlap"),
                     (dict(t_out=ptr, t_out_stride=43, obs_dim=33), b"without terminal_obs")):
        assert lib.qg_sched_advance_device(*args(**kw)) == -1 and word in lib.qg_last_error(), (kw, lib.qg_last_error())
    assert lib.qg_sched_begin_device(sched._h, None, ptr, 42, 33, None) == -1 and b"row_stride" in lib.qg_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(sensor.state(), before) and np.array_equal(sched.state(), s_before) and not wide.any()    # nothing was launched
    _close(sched, sensor, sim)
    # terminal_out with done_row = terminal: refused on both sides of the binding
    sim, sensor, sched = _loaded(fix, slice(0, n))
    with pytest.raises(ValueError, match="done_row='reset'"):
        sched.step(terminal_out=z(n, 10))
    assert lib.qg_sched_advance_device(*[dict(names, h=sched._h, t_out=ptr, t_out_stride=10)[k] for k, _ in names]) == -1
    assert b"QG_PERTURB_DONE_ROW_RESET" in lib.qg_last_error()
    # a snapshot of another shape is refused
    with pytest.raises(ValueError):
        sched.load_state(np.zeros(10, np.uint8))
    _close(sched, sensor, sim)


def test_refused_in_resident_mode_and_above_half_a_period_per_step():
    n = 64
    sim = BatchedSim(n, task=_task(walk=True))
    sim.reset(seed=2)
    sensor = ContactSensor(sim, R.FORCE_THRESHOLD)
    sched = GaitSchedule(sensor, R.TABLE, R.FREQ, R.WEIGHTS, **OPTS)
    s0 = sched.state()
    mail_a, mail_p = torch.zeros((2, n, 12), device=DEV), torch.zeros((2, n, 35), device=DEV)
    sim.resident_start(mail_a, mail_p)
    with pytest.raises(_abi.QuadGymError, match="qg_resident_stop first"):
        sched.step()
    sim.resident_stop()
    assert np.array_equal(sched.state(), s0)
    # freq_hi x dt: 3 Hz x 0.2 s = 0.6 of a period per env-step
    sim.set_task(_task(frame_skip=100, walk=True))
    with pytest.raises(_abi.QuadGymError, match="> 0.5"):
        sched.step()
    assert np.array_equal(sched.state(), s0)
    sim.set_task(_task(frame_skip=83, walk=True))                                   # 3 Hz x 0.166 s = 0.498: the largest step that passes
    comps, out, _ = sched.step()
    torch.cuda.synchronize()
    assert torch.isfinite(comps).all() and torch.isfinite(out).all() and not np.array_equal(sched.state(), s0)
    _close(sched, sensor, sim)
