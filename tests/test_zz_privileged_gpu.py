"""The privileged state pack on the GPU (qg_priv_*, csrc/qg_priv.hip): on the built contact states the copy-through columns are the
bits qg_get_state / qg_get_dynamics / qg_get_xfrc return, the foot columns the bits of ContactSensor.read, the two rotated columns
within MARGIN x the measured float32 budget of the float64 definition (tests/privileged_reference.py); the modes (dynamics rows,
wrench rows, the push schedule: the reported wrench given to a twin as explicit rows steps it bit for bit like the scheduled handle);
the observation in front bit for bit from contiguous and strided sources, sentinels around the rows, rows independent of the handle's
size, graph replay, invisibility to the simulator, the refusals, and the VecEnv wrapper.
The module's name puts it last in collection, as the other modules that capture hipGraphs on a side stream."""
import numpy as np
import pytest
import torch

import contact_cells as CC
import contact_sensor_reference as CR
import privileged_reference as P

from quadruped_gym_amd import _abi
from quadruped_gym_amd.contact import ContactSensor
from quadruped_gym_amd.privileged import DevicePrivilegedVecEnv, PrivilegedState
from quadruped_gym_amd.sim import BatchedSim

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COL = P.COL
SENTINEL = -7.25
PUSH = {"interval": 3, "duration": 2, "probability": 0.6, "force": (4.0, 12.0)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def fix():
    return CC.load()


def _loaded(fix, idx=None, threshold=0.0):
    """(sim, pack) holding the fixture states `idx` (all: None)."""
    idx = np.arange(len(fix["qpos"])) if idx is None else np.asarray(idx)
    sim = BatchedSim(len(idx))
    sim.set_state(fix["qpos"][idx], fix["qvel"][idx], fix["act"][idx], None, fix["nstep"][idx])
    return sim, PrivilegedState(sim, threshold)


def _read(pack, obs=None, pad=0):
    """The rows of one read into a sentinel-filled [N, O + 85 + pad] buffer, as NumPy."""
    width = (0 if obs is None else obs.shape[1]) + P.DIM
    buf = torch.full((pack.num_envs, width + pad), SENTINEL, device=DEV)
    pack.read(buf[:, :width] if pad else buf, obs)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.fixture(scope="module")
def full_read(fix):
    """One handle of all 664 states (not a multiple of 16), threshold 1 N: shared, and left unchanged."""
    sim, pack = _loaded(fix, threshold=1.0)
    rows = _read(pack)
    host = pack.read_host()
    pack.close(), sim.close()
    assert np.array_equal(bits(rows), bits(host))              # the synchronous read is the same launch
    rows.setflags(write=False)
    return rows


def _check_against_the_simulator(rows, sim, threshold):
    """The 85 columns `rows` of `sim`'s state: copies bit for bit, the foot columns the sensor's bits, the count the sensor's forces'."""
    qpos, qvel, act, _, nstep = sim.get_state()
    want = {"base_ang_vel": qvel[:, 3:6], "base_height": qpos[:, 2:3], "joint_pos": qpos[:, 7:19], "joint_vel": qvel[:, 6:18], "act": act,
            "dynamics": sim.get_dynamics()}
    assert set(want) == set(P.COPIES)
    for name, value in want.items():
        assert np.array_equal(bits(rows[:, COL[name]]), bits(value)), name
    sensor = ContactSensor(sim, threshold)
    force, feet = sensor.read_host()
    sensor.close()
    n = len(rows)
    assert np.array_equal(bits(rows[:, COL["foot_contact"]]), bits(feet[:, :, 6]))
    assert np.array_equal(bits(rows[:, COL["foot_force"]]), bits(force[:, list(CR.FEET)].reshape(n, 12)))
    assert np.array_equal(bits(rows[:, COL["foot_height"]]), bits(feet[:, :, 2]))
    assert np.array_equal(rows[:, COL["body_contact"]][:, 0], (force[:, P.NON_FOOT, 2] > np.float32(threshold)).sum(1))
    assert np.array_equal(bits(rows[:, COL["episode_time"]][:, 0]), bits(nstep.astype(np.float32) * np.float32(sim.model.timestep)))
    return qpos, qvel, force


def _check_rotated(what, rows, qpos, qvel):
    lin64, g64 = P.base_columns(qpos, qvel)
    for name, want, budget in (("base_lin_vel", lin64, P.BUDGET_BASE_LIN_VEL), ("gravity_dir", g64, P.BUDGET_GRAVITY_DIR)):
        err = rows[:, COL[name]].astype(np.float64) - want
        share = CR.share(err, budget, want) / CR.MARGIN
        print("%s: %-12s largest |gpu - f64| %.3e, largest share of %.0f x (%.1e + %.1e |f64|): %.3f"
              % (what, name, np.abs(err).max(), CR.MARGIN, *budget, share))
        assert share <= 1.0, (name, share)


# ---- 1. the columns on the built contact states ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(1, 663), (5, 100), (67, 300)])
def test_fixture_columns(oracle, fix, full_read, n, k):
    idx = np.arange(k, k + n)
    sim, pack = _loaded(fix, idx, threshold=1.0)
    rows = _read(pack)
    assert rows.shape == (n, 85) and np.isfinite(rows).all()
    qpos, qvel, force = _check_against_the_simulator(rows, sim, 1.0)
    assert np.array_equal(bits(qpos), bits(fix["qpos"][idx]))
    _check_rotated("%d states" % n, rows, qpos, qvel)
    assert not rows[:, COL["frame_wrench"]].any()              # wrench mode is off
    assert np.array_equal(rows[:, COL["dynamics"]], np.tile(_abi.identity_dynamics_row(sim.model), (n, 1)))
    # rows depend on their env alone: a handle of 664 computes the same bits
    assert np.array_equal(bits(rows), bits(full_read[k:k + n]))
    pack.close(), sim.close()


def test_all_states_against_the_definition(oracle, fix, full_read):
    """The 664 rows against tests/privileged_reference.py in float64: forces within the sensor's budgets, flags outside its band."""
    model = oracle.default_model()
    want, ref = P.evaluate(model, fix["qpos"], fix["qvel"], fix["act"], fix["nstep"], threshold=1.0)
    _check_rotated("664 states", full_read, fix["qpos"], fix["qvel"])
    feet = list(CR.FEET)
    got_force = full_read[:, COL["foot_force"]].reshape(-1, 4, 3).astype(np.float64)
    for name, got, exp, budget in (("normal", got_force[..., 2], ref["force"][:, feet, 2], CR.BUDGET_FORCE_NORMAL),
                                   ("tangential", got_force[..., :2], ref["force"][:, feet, :2], CR.BUDGET_FORCE_TANGENTIAL),
                                   ("foot height", full_read[:, COL["foot_height"]].astype(np.float64), ref["foot_pos"][..., 2], CR.BUDGET_FOOT_POS)):
        share = CR.share(got - exp, budget, exp) / CR.MARGIN
        print("664 states: %-11s largest share of the sensor's bound: %.3f" % (name, share))
        assert share <= 1.0, (name, share)
    band = CR.flag_band(ref, 1.0)
    assert band.sum() <= CR.MAX_EXCLUDED * band.size
    flags = full_read[:, COL["foot_contact"]]
    assert set(np.unique(flags)) <= {0.0, 1.0} and 0 < flags.sum() < flags.size
    assert not ((flags != want[:, COL["foot_contact"]]) & ~band[:, feet]).any()
    quiet = ~band[:, P.NON_FOOT].any(1)
    assert np.array_equal(full_read[quiet, COL["body_contact"]], want[quiet, COL["body_contact"]]) and full_read[:, 66].max() >= 1
    for name in ("base_ang_vel", "base_height", "joint_pos", "joint_vel", "act", "dynamics", "frame_wrench", "episode_time"):
        assert np.array_equal(full_read[:, COL[name]], want[:, COL[name]].astype(np.float32)), name


# ---- 2. the modes -------------------------------------------------------------------------------------------------------------------------
def test_explicit_dynamics_and_wrench_rows(oracle, fix):
    rng = np.random.default_rng(11)
    n = 67
    idx = np.sort(rng.choice(664, n, replace=False))
    sim, pack = _loaded(fix, idx, threshold=0.0)
    plain = _read(pack)
    rows = np.tile(_abi.identity_dynamics_row(sim.model), (n, 1))
    rows[:, 0], rows[:, 1], rows[:, 5:] = rng.uniform(0.3, 1.5, n), rng.uniform(0, 0.5, n), rng.uniform(0.6, 1.6, (n, 6))
    sim.set_dynamics(rows)
    got = _read(pack)
    _check_against_the_simulator(got, sim, 0.0)
    assert np.array_equal(bits(got[:, COL["dynamics"]]), bits(rows)) and not got[:, COL["frame_wrench"]].any()
    assert np.abs(got[:, COL["foot_force"]] - plain[:, COL["foot_force"]]).max() > 1.0        # the rows reach the forces
    xfrc = rng.uniform(-3, 3, (n, 13, 6)).astype(np.float32)
    sim.set_external_wrench(xfrc)
    both = _read(pack)
    assert np.array_equal(bits(both[:, COL["frame_wrench"]]), bits(sim.get_external_wrench()[:, 0]))
    assert np.array_equal(bits(both[:, COL["frame_wrench"]]), bits(xfrc[:, 0]))
    assert np.array_equal(bits(both[:, :78]), bits(got[:, :78])) and np.array_equal(bits(both[:, 84]), bits(got[:, 84]))
    sim.clear_dynamics()                                       # wrench mode alone: identity rows again, the wrench stays
    alone = _read(pack)
    assert np.array_equal(bits(alone[:, COL["dynamics"]]), bits(plain[:, COL["dynamics"]]))
    assert np.array_equal(bits(alone[:, COL["frame_wrench"]]), bits(xfrc[:, 0]))
    assert np.array_equal(bits(alone[:, :67]), bits(plain[:, :67]))
    sim.clear_external_wrench()
    assert np.array_equal(bits(_read(pack)), bits(plain))
    pack.close(), sim.close()


def test_push_schedule_is_reported_and_a_twin_given_the_rows_steps_alike(fix):
    """Two episodes of seven env-steps: the reported force is the reference's push for (seed, env, episode, nstep / frame_skip) on top
    of the FRAME's own row, and a twin without a schedule that gets the reported wrench as its FRAME row steps bit for bit alike."""
    n, base = 67, 1000
    rng = np.random.default_rng(75)
    idx = np.sort(rng.choice(664, n, replace=False))
    sim, twin = BatchedSim(n, env_index_base=base), BatchedSim(n, env_index_base=base)
    pack = PrivilegedState(sim)
    own = np.zeros((n, 13, 6), np.float32)
    own[:, 0] = rng.uniform(-1, 1, (n, 6))
    sim.set_external_wrench(own), sim.set_push_schedule(PUSH)
    twin.set_external_wrench(own)
    fs = sim.get_task().frame_skip
    held = []
    for episode in range(2):
        sim.reset(seed=21), twin.reset(seed=21)
        state = (fix["qpos"][idx], fix["qvel"][idx], fix["act"][idx], None, np.zeros(n, np.int32))
        sim.set_state(*state), twin.set_state(*state)
        for t in range(7):
            rows = pack.read_host()
            ep, seed = sim.get_reset_streams()
            nstep = sim.get_state()[4]
            assert seed == 21
            want = np.array([P.push_force(PUSH, seed, base + i, ep[i], nstep[i] // fs) for i in range(n)])
            got = rows[:, COL["frame_wrench"]].astype(np.float64) - own[:, 0]
            assert np.abs(got[:, :2] - want).max() <= P.PUSH_RTOL * PUSH["force"][1] + 2.0 ** -21      # (the f32 sum with the own row: half an ulp at |x| < 16)
            assert np.array_equal(np.abs(got[:, :2]).sum(1) > 1e-3, np.abs(want).sum(1) > 0)
            assert np.array_equal(bits(rows[:, 80:84]), bits(own[:, 0, 2:]))                       # z force and torque: the row's bits
            assert np.array_equal(bits(rows[:, 84]), bits(nstep.astype(np.float32) * np.float32(sim.model.timestep)))
            held.append(np.abs(want).sum(1) > 0)
            given = own.copy()
            given[:, 0] = rows[:, COL["frame_wrench"]]
            twin.set_external_wrench(given)
            acts = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
            a, b = sim.step(acts), twin.step(acts)
            for x, y in zip(a[:3] + sim.get_state(), b[:3] + twin.get_state()):
                assert np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y), (episode, t)
    assert 0.1 < np.mean(held) < 0.7 and (np.array(held[:7]) != np.array(held[7:])).any()
    pack.close(), sim.close(), twin.close()


# ---- 3. the observation in front, sentinels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 67])
def test_observation_is_copied_bit_for_bit(fix, full_read, n):
    sim, pack = _loaded(fix, np.arange(300, 300 + n), threshold=1.0)
    want = full_read[300:300 + n]
    gen = torch.Generator(device=DEV).manual_seed(3)
    packed = torch.randn((n, 35), device=DEV, generator=gen)
    packed[0, 0], packed[n - 1, 32] = float("nan"), -0.0        # bits, not values
    sources = {"contiguous 33": packed[:, :33].contiguous(), "packed rows 33": packed[:, :33],
               "16-byte path 260": torch.randn((n, 260), device=DEV, generator=gen),
               "260 at stride 264": torch.randn((n, 264), device=DEV, generator=gen)[:, :260],
               "odd pointer 12": torch.randn((n * 12 + 1), device=DEV, generator=gen)[1:].view(n, 12), "one column": packed[:, 34:35]}
    for what, obs in sources.items():
        O = obs.shape[1]
        pad = 3                                                 # (260 + 85 + 3 = 348: the 16-byte path needs an out stride that is a multiple of 4)
        whole = torch.full((n + 2, O + 85 + pad), SENTINEL, device=DEV)      # a row of another tensor's on either side
        out = whole[1:n + 1, :O + 85]
        before = obs.clone()
        assert pack.read(out, obs) is out
        torch.cuda.synchronize()
        got = whole.cpu().numpy()
        assert np.array_equal(bits(got[1:n + 1, :O]), bits(obs.cpu().numpy())), what
        assert np.array_equal(bits(got[1:n + 1, O:O + 85]), bits(want)), what
        assert (got[0] == SENTINEL).all() and (got[n + 1] == SENTINEL).all() and (got[1:n + 1, O + 85:] == SENTINEL).all(), what
        assert np.array_equal(bits(obs.cpu().numpy()), bits(before.cpu().numpy())), what
    pack.close(), sim.close()


# ---- 4. graph replay, invisibility, refusals -----------------------------------------------------------------------------------------------
def _walk_task():
    t = _abi.default_task()
    t.auto_reset, t.use_time_limit, t.max_time, t.use_fall, t.use_flip = 1, 1, 0.04, 0, 0     # 5 env-steps per episode
    return t


def test_graph_replay_is_the_eager_run():
    """The env-step and the pack behind it, captured once and replayed 8 times, against 8 eager steps of a twin; auto-resets included:
    the rows of a finished env describe the new episode's first state."""
    n = 67
    acts = torch.tensor(np.random.default_rng(3).uniform(-1, 1, (8, n, 12)).astype(np.float32)).to(DEV)

    def make():
        sim = BatchedSim(n, task=_walk_task())
        sim.set_push_schedule(PUSH)
        sim.reset(seed=1)
        return sim, PrivilegedState(sim, 1.0), torch.zeros((n, 35), device=DEV), torch.zeros((n, 33 + 85), device=DEV)

    sim, pack, packed, wide = make()
    eager = []
    for t in range(8):
        sim.step_device_packed(acts[t], packed)
        pack.read(wide, packed[:, :33])
        torch.cuda.synchronize()
        eager.append(wide.cpu().numpy().copy())
        if packed[:, 34].any():                                 # the finished envs were reset: time 0, the start pose's height
            assert (eager[-1][packed[:, 34].cpu().numpy() != 0, 33 + 84] == 0).all()
    assert any((e[:, 33 + 84] == 0).any() for e in eager) and any(e[:, 33 + 78:33 + 80].any() for e in eager)
    assert np.array_equal(eager[2][:, 33 + 84], np.full(n, np.float32(12) * np.float32(sim.model.timestep)))
    pack.close(), sim.close()

    sim, pack, packed, wide = make()
    snap = sim.snapshot()
    s_act = torch.zeros((n, 12), device=DEV)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        sim.step_device_packed(s_act, packed, stream=side)
        pack.read(wide, packed[:, :33], stream=side)
    sim.restore(snap)                                           # whatever a capture may have run, start from the fresh state
    for t in range(8):
        s_act.copy_(acts[t])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(wide.cpu().numpy()), bits(eager[t])), t
    del graph
    pack.close(), sim.close()


def test_refused_in_resident_mode_and_invisible_to_the_simulator():
    n = 64
    a, b = BatchedSim(n, task=_walk_task()), BatchedSim(n, task=_walk_task())
    a.reset(seed=2), b.reset(seed=2)
    pack = PrivilegedState(a)
    out = torch.zeros((n, 85), device=DEV)
    mail_a, mail_p = torch.zeros((2, n, 12), device=DEV), torch.zeros((2, n, 35), device=DEV)
    a.resident_start(mail_a, mail_p)
    with pytest.raises(_abi.QuadGymError, match="qg_resident_stop first"):
        pack.read(out)
    with pytest.raises(_abi.QuadGymError, match="qg_resident_stop first"):
        pack.read_host()
    a.resident_stop()
    assert not out.any()
    # a step, then a read, leaves the simulator's next step bit-identical to a twin that never read
    acts = torch.tensor(np.random.default_rng(9).uniform(-1, 1, (12, n, 12)).astype(np.float32)).to(DEV)
    pa, pb = torch.zeros((n, 35), device=DEV), torch.zeros((n, 35), device=DEV)
    for t in range(12):
        a.step_device_packed(acts[t], pa), b.step_device_packed(acts[t], pb)
        pack.read(out)
        torch.cuda.synchronize()
        assert torch.equal(pa, pb) and torch.isfinite(out).all(), t
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    pack.close(), a.close(), b.close()


def test_bad_tensors_raise_before_any_launch(fix):
    sim, pack = _loaded(fix, np.arange(8))
    out = torch.full((8, 118), SENTINEL, device=DEV)
    obs = torch.zeros((8, 33), device=DEV)
    bad = [dict(out=out.double(), obs=obs), dict(out=out.cpu(), obs=obs), dict(out=out, obs=obs.half()), dict(out=out[:, :117], obs=obs),
           dict(out=out, obs=None), dict(out=torch.zeros((9, 118), device=DEV), obs=obs), dict(out=out, obs=torch.zeros((7, 33), device=DEV)),
           dict(out=torch.zeros((118, 8), device=DEV).t(), obs=obs), dict(out=out, obs=torch.zeros((8, 66), device=DEV)[:, ::2]),
           dict(out=out, obs=out[:, :33]), dict(out=out.view(-1)[: 8 * 85], obs=None)]
    for kw in bad:
        with pytest.raises(ValueError):
            pack.read(**kw)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    lib = _abi.load_library()
    assert lib.qg_priv_read_device(pack._h, obs.data_ptr(), 33, 33, obs.data_ptr() + 4 * 16, 118, None) == -1 and b"overlap" in lib.qg_last_error()
    assert lib.qg_priv_read_device(pack._h, None, 0, 0, out.data_ptr(), 84, None) == -1
    assert (out == SENTINEL).all()
    pack.read(out, obs)                                          # and a good one
    torch.cuda.synchronize()
    assert (out[:, :33] == 0).all() and (out[:, 33:] != SENTINEL).all()
    pack.close(), sim.close()


# ---- 5. the VecEnv wrapper ---------------------------------------------------------------------------------------------------------------
def test_wrapper_around_the_plain_and_the_walking_env():
    from quadruped_gym_amd.envs.vec_env import QuadrupedVecEnv
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
    n = 64
    acts = torch.tensor(np.random.default_rng(4).uniform(-1, 1, (3, n, 12)).astype(np.float32)).to(DEV)
    # the plain env: packed rows come back as they do from the env, the wide rows through the keyword
    env = DevicePrivilegedVecEnv(QuadrupedVecEnv(n, push_randomization={"interval_s": 0.024, "duration_s": 0.016, "probability": 0.7, "force": (2, 6)}), 1.0)
    twin = QuadrupedVecEnv(n, push_randomization={"interval_s": 0.024, "duration_s": 0.016, "probability": 0.7, "force": (2, 6)})
    assert (env.obs_dim, env.actor_obs_dim, env.privileged_dim) == (118, 33, 85) and env.observation_space.shape == (118,)
    assert env.privileged is env.venv.privileged_state(1.0)
    with pytest.raises(ValueError):
        env.venv.privileged_state(2.0)
    first = env.reset()
    twin.reset()
    assert first.shape == (n, 118) and not first[:, :33].any() and (first[:, 33 + 84] == 0).all() and (first[:, 33 + 6:33 + 9] == [0, 0, -1]).all()
    wide = torch.zeros((n, 118), device=DEV)
    for t in range(3):
        packed, want = env.step_tensor(acts[t], wide=wide), twin.step_tensor(acts[t])
        torch.cuda.synchronize()
        assert torch.equal(packed, want) and torch.equal(wide[:, :33], packed[:, :33])
        assert np.array_equal(bits(wide[:, 33:].cpu().numpy()), bits(env.privileged.read_host()))
    obs, rew, done, infos = env.step(acts[0].cpu().numpy())      # the NumPy cold path returns wide rows
    assert obs.shape == (n, 118) and rew.shape == (n,) and np.array_equal(bits(obs[:, 33:]), bits(env.privileged.read_host()))
    pack = env.privileged
    env.close(), twin.close()
    assert pack._h is None                                       # closed with the env
    # the partially observable walking env: obs is [N, 52 + 85]; the terminal rows stay at the actor's width
    env = DevicePrivilegedVecEnv(POWalkingQuadrupedVecEnv(n, obs_window=2, max_time=0.02), 0.0)
    twin = POWalkingQuadrupedVecEnv(n, obs_window=2, max_time=0.02)
    env.reset(), twin.reset()
    O = env.actor_obs_dim
    assert O == 52 and env.obs_dim == 137
    bufs = lambda w: [torch.zeros((n, w), device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV, dtype=torch.uint8)]
    (wide, rew, done), (obs, rew2, done2) = bufs(137), bufs(52)
    term, term2 = torch.zeros((n, 52), device=DEV), torch.zeros((n, 52), device=DEV)
    finished = 0
    for t in range(3):
        env.step_tensor(acts[t], wide, rew, done, terminal_obs=term)
        twin.step_tensor(acts[t], obs, rew2, done2, terminal_obs=term2)
        torch.cuda.synchronize()
        same = lambda x, y: torch.equal(x.contiguous().view(torch.int32), y.view(torch.int32))       # bits: a reward may be NaN
        assert same(wide[:, :O], obs) and same(rew, rew2) and torch.equal(done, done2) and same(term, term2)
        assert np.array_equal(bits(wide[:, O:].cpu().numpy()), bits(env.privileged.read_host()))
        finished += int(done.sum())
    assert finished > 0
    with pytest.raises(ValueError):
        env.step_tensor(acts[0], obs, rew, done)                # the narrow buffer: refused before the env's launch
    env.close(), twin.close()


def test_documented_stacking_around_the_walking_env():
    """INTEGRATION.md section 20's order: DevicePerturbedVecEnv inside, DevicePrivilegedVecEnv, DeviceVecNormalize outside, around
    WalkingQuadrupedVecEnv.  Sensor noise moves the actor's columns and leaves the privileged ones clean (bit for bit a noise-free
    twin's); the normaliser outside sees the wide row; everything passes through two wrappers."""
    from quadruped_gym_amd.envs.walking import WalkingQuadrupedVecEnv
    from quadruped_gym_amd.normalize import DeviceVecNormalize
    from quadruped_gym_amd.perturb import DevicePerturbedVecEnv
    n = 64
    acts = torch.tensor(np.random.default_rng(8).uniform(-1, 1, (3, n, 12)).astype(np.float32)).to(DEV)
    make = lambda: WalkingQuadrupedVecEnv(n, nan_direction=False, random_controls=True, device_commands=True)
    noisy = DevicePrivilegedVecEnv(DevicePerturbedVecEnv(make(), obs_noise=0.1, seed=3), 1.0)
    clean = DevicePrivilegedVecEnv(make(), 1.0)
    stack = DeviceVecNormalize(DevicePrivilegedVecEnv(DevicePerturbedVecEnv(make(), obs_noise=0.1, seed=3), 1.0))
    assert noisy.obs_dim == clean.obs_dim == stack.obs_dim == 118 and stack.normalizer.obs_dim == 118 and stack.actor_obs_dim == 33
    assert noisy.privileged is noisy.venv.venv.privileged_state(1.0) and not noisy._packed
    for env in (noisy, clean, stack):
        assert env.reset().shape == (n, 118)
    bufs = lambda: [torch.zeros((n, 118), device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV, dtype=torch.uint8)]
    (w_n, r_n, d_n), (w_c, r_c, d_c), (w_s, r_s, d_s) = bufs(), bufs(), bufs()
    for t in range(3):
        noisy.step_tensor(acts[t], w_n, r_n, d_n), clean.step_tensor(acts[t], w_c, r_c, d_c), stack.step_tensor(acts[t], w_s, r_s, d_s)
        torch.cuda.synchronize()
        assert torch.equal(w_n[:, 33:], w_c[:, 33:]) and torch.equal(d_n, d_c)       # the truth is untouched by the sensors' noise
        assert (w_n[:, :33] != w_c[:, :33]).float().mean() > 0.5                    # ... which is on the actor's columns
        assert np.array_equal(bits(w_n[:, 33:].cpu().numpy()), bits(noisy.privileged.read_host()))
        # the normaliser outside: the same wide row, normalised -- finite, changed, and clipped to its +-10
        assert torch.isfinite(w_s).all() and not torch.equal(w_s, w_n) and w_s.abs().max() <= 10.0
    mean = stack.normalizer.state_dict()
    assert any(np.asarray(v).shape == (118,) for v in mean.values())             # statistics over the wide row
    for env in (noisy, clean, stack):
        env.close()
