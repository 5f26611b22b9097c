"""The contact sensor on the GPU (qg_contact_*, csrc/qg_contact.hip) against the float64 definition of tests/contact_sensor_reference.py:
forces and foot kinematics within MARGIN x the measured float32 budget on the 664 built contact states, flags equal outside the
exclusion band, per-env dynamics and another model against the oracle's models, rows independent of the handle's size bit for bit,
integer timers exact through touchdowns, liftoffs and auto-resets, state / snapshot / graph replay bit for bit, and the refusals.
With QG_CONTACT_PARITY_OUT=<file> the parity cases append their largest errors as shares of the bound (profiles/r25).
The module's name puts it last in collection, as the other modules that capture hipGraphs on a side stream: the resident-mode tests
of the modules before it find the process's streams as they were."""
import os

import numpy as np
import pytest
import torch

import contact_cells as CC
import contact_sensor_reference as R
from helpers import env_model, table_model

from quadruped_gym_amd import _abi
from quadruped_gym_amd.contact import ContactSensor
from quadruped_gym_amd.sim import BatchedSim

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FEET = list(R.FEET)


def _record(line):
    print(line)
    out = os.environ.get("QG_CONTACT_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


@pytest.fixture(scope="module")
def fix():
    return CC.load()


@pytest.fixture(scope="module")
def ref(oracle, fix):
    return R.evaluate(oracle.default_model(), fix["qpos"], fix["qvel"])


def _loaded(fix, idx=None, model=None, threshold=0.0):
    """(sim, sensor) holding the fixture states `idx` (all: None)."""
    idx = np.arange(len(fix["qpos"])) if idx is None else np.asarray(idx)
    sim = BatchedSim(len(idx), model=model)
    sim.set_state(fix["qpos"][idx], fix["qvel"][idx], fix["act"][idx], None, fix["nstep"][idx])
    return sim, ContactSensor(sim, threshold)


def _read(sensor, **kw):
    force, feet = sensor.read(advance=False, **kw)
    torch.cuda.synchronize()
    return force.cpu().numpy(), feet.cpu().numpy()


@pytest.fixture(scope="module")
def full_read(fix):
    """The non-advancing read of one handle of all 664 states (not a multiple of 16): shared, and left unchanged."""
    sim, sensor = _loaded(fix)
    force, feet = _read(sensor)
    blob = sensor.state()
    sensor.close(), sim.close()
    force.setflags(write=False), feet.setflags(write=False)
    return force, feet, blob


def _check_parity(what, force, feet, ref, threshold=0.0):
    """Forces and foot kinematics within MARGIN x BUDGET; flags equal outside the band (the share left out is asserted)."""
    cases = (("force normal", force[..., 2], ref["force"][..., 2], R.BUDGET_FORCE_NORMAL),
             ("force tangential", force[..., :2], ref["force"][..., :2], R.BUDGET_FORCE_TANGENTIAL),
             ("foot position", feet[..., 0:3], ref["foot_pos"], R.BUDGET_FOOT_POS),
             ("foot velocity", feet[..., 3:6], ref["foot_vel"], R.BUDGET_FOOT_VEL))
    shares = {}
    for name, got, want, budget in cases:
        err = got.astype(np.float64) - want
        shares[name] = R.share(err, budget, want) / R.MARGIN
        _record("%s: %-17s largest |gpu - f64| %.3e, largest share of %.0f x (%.1e + %.1e |f64|): %.3f"
                % (what, name, np.abs(err).max(), R.MARGIN, budget[0], budget[1], shares[name]))
    band = R.flag_band(ref, threshold)
    want_flags = R.flags(ref["force"], threshold)
    got_flags = force[..., 2] > np.float32(threshold)
    _record("%s: flags left out %d of %d pairs; feet in contact %d" % (what, int(band.sum()), band.size, int(feet[..., 6].sum())))
    assert band.sum() <= R.MAX_EXCLUDED * band.size
    assert all(s <= 1.0 for s in shares.values()), shares
    assert not ((got_flags != want_flags) & ~band).any()
    assert set(np.unique(feet[..., 6:9])) <= {0.0, 1.0}
    assert not ((feet[..., 6] != want_flags[:, FEET]) & ~band[:, FEET]).any()
    assert np.array_equal(feet[..., 6] > 0.5, got_flags[:, FEET])               # the column is the flag of the force it reports


# ---- 1. parity ----------------------------------------------------------------------------------------------------------------------------
def test_fixture_parity(fix, ref, full_read):
    force, feet, blob = full_read
    assert force.shape == (664, 13, 3) and feet.shape == (664, 4, 12) and (fix["kind"] == CC.KIND_EDGE).sum() > 0
    _check_parity("664 states", force, feet, ref)
    # a fresh handle, no advancing read: no event, zero times, and nothing written
    assert not feet[..., 7:].any()
    assert not np.frombuffer(blob.tobytes()[24:], np.int32).any()


def test_threshold(fix, ref, full_read):
    sim, sensor = _loaded(fix, threshold=5.0)
    force, feet = _read(sensor)
    sensor.close(), sim.close()
    assert np.array_equal(force.view(np.uint32), full_read[0].view(np.uint32))  # the threshold moves the flags alone
    _check_parity("threshold 5 N", force, feet, ref, threshold=5.0)
    assert 0 < feet[..., 6].sum() < full_read[1][..., 6].sum()


def test_per_env_dynamics(oracle, fix):
    """128 states that touch, each with its own friction and contact stiffness / damping scales, against the oracle's model per env."""
    rng = np.random.default_rng(7)
    base = oracle.default_model()
    touching = np.flatnonzero(R.evaluate(base, fix["qpos"], fix["qvel"])["W"].sum(1) > 0)
    idx = np.sort(rng.choice(touching, 128, replace=False))
    rows = np.tile(_abi.identity_dynamics_row(base), (128, 1))
    rows[:, 0], rows[:, 9], rows[:, 10] = rng.uniform(0.3, 1.5, 128), rng.uniform(0.6, 1.6, 128), rng.uniform(0.5, 1.8, 128)
    sim, sensor = _loaded(fix, idx)
    sim.set_dynamics(rows)
    force, feet = _read(sensor)
    sensor.close(), sim.close()
    keys = ("force", "foot_pos", "foot_vel", "W", "gap", "normal_unclipped")
    parts = [R.evaluate(env_model(oracle, base, rows[i]), fix["qpos"][idx[i]][None], fix["qvel"][idx[i]][None]) for i in range(128)]
    want = {k: np.concatenate([p[k] for p in parts]) for k in keys}
    # the restatement with a row is the restatement on that env's model, and the oracle's force on that model
    with_rows = R.evaluate(base, fix["qpos"][idx], fix["qvel"][idx], rows=rows.astype(np.float64))
    assert np.abs(with_rows["force"] - want["force"]).max() < 1e-9
    e = oracle.make_env(fix["qpos"][idx[0]], fix["qvel"][idx[0]], fix["act"][idx[0]])
    _, dg = oracle.substep(env_model(oracle, base, rows[0]), e, np.zeros(12), want_diag=True)
    assert np.abs(np.array([list(r) for r in dg.contact_F]) - want["force"][0]).max() < 1e-9
    _check_parity("per-env dynamics", force, feet, want)
    assert np.abs(force - full_rows(fix, idx)).max() > 1.0                      # the rows matter


def full_rows(fix, idx):
    sim, sensor = _loaded(fix, idx)
    force, _ = _read(sensor)
    sensor.close(), sim.close()
    return force


def test_generic_model(oracle, fix):
    """The table robot (contact stiffness -10 %): the constants come from the handle's model."""
    model = table_model(oracle.default_model())
    idx = np.arange(0, 664, 5)[:128]
    sim, sensor = _loaded(fix, idx, model=table_model(_abi.default_model()))
    assert not sim.baked
    force, feet = _read(sensor)
    sensor.close(), sim.close()
    want = R.evaluate(model, fix["qpos"][idx], fix["qvel"][idx])
    e = oracle.make_env(fix["qpos"][idx[3]], fix["qvel"][idx[3]], fix["act"][idx[3]])
    _, dg = oracle.substep(model, e, np.zeros(12), want_diag=True)
    assert np.abs(np.array([list(r) for r in dg.contact_F]) - want["force"][3]).max() < 1e-9
    _check_parity("table robot", force, feet, want)


@pytest.mark.parametrize("n,k", [(1, 663), (3, 100), (17, 400)])
def test_rows_do_not_depend_on_the_handle(fix, full_read, n, k):
    sim, sensor = _loaded(fix, np.arange(k, k + n))
    force, feet = _read(sensor)
    sensor.close(), sim.close()
    assert np.array_equal(force.view(np.uint32), full_read[0][k:k + n].view(np.uint32))
    assert np.array_equal(feet.view(np.uint32), full_read[1][k:k + n].view(np.uint32))


# ---- 2. timers ------------------------------------------------------------------------------------------------------------------------------
N_WALK, T_WALK = 67, 80


def _walk_task():
    t = _abi.default_task()
    t.auto_reset, t.use_time_limit, t.max_time, t.use_fall, t.use_flip = 1, 1, 0.2, 0, 0     # 25 env-steps per episode
    return t


def _actions(seed=3):
    return torch.tensor(np.random.default_rng(seed).uniform(-1, 1, (T_WALK, N_WALK, 12)).astype(np.float32)).to(DEV)


class _Run:
    """A simulator with a sensor, stepped on the shared actions; every step returns the bits of everything the step and the read wrote."""

    def __init__(self):
        self.sim = BatchedSim(N_WALK, task=_walk_task())
        self.sim.reset(seed=1)
        self.sensor = ContactSensor(self.sim)
        self.packed = torch.zeros((N_WALK, 35), device=DEV)
        self.force = torch.zeros((N_WALK, 13, 3), device=DEV)
        self.feet = torch.zeros((N_WALK, 4, 12), device=DEV)

    def step(self, actions):
        self.sim.step_device_packed(actions, self.packed)
        self.sensor.read(done=self.packed[:, 34], body_force=self.force, feet=self.feet)

    def bits(self):
        torch.cuda.synchronize()
        return np.concatenate([t.cpu().numpy().view(np.uint32).ravel() for t in (self.packed, self.force, self.feet)])

    def close(self):
        self.sensor.close(), self.sim.close()


@pytest.fixture(scope="module")
def walk():
    """The eager run: per step the output bits, the feet rows and done; the sensor's state at step 40 and at the end."""
    run, acts = _Run(), _actions()
    bits, feet, done, mid = [], [], [], None
    for t in range(T_WALK):
        if t == 40:
            mid = (run.sensor.state(), run.sim.snapshot())
        run.step(acts[t])
        bits.append(run.bits())
        feet.append(run.feet.cpu().numpy()), done.append(run.packed[:, 34].cpu().numpy() != 0)
    end = run.sensor.state()
    run.close()
    return dict(bits=bits, feet=np.stack(feet), done=np.stack(done), mid=mid, end=end)


def test_timers_are_the_integer_reference(walk):
    dt = np.float32(_abi.default_model().timestep * 4)
    timers = R.Timers(N_WALK)
    feet, done = walk["feet"], walk["done"]
    for t in range(T_WALK):
        td, lo = timers.advance(feet[t, :, :, 6] > 0.5, done[t])
        ph, air, st = timers.times(dt)
        for col, want in ((7, td), (8, lo), (9, ph), (10, air), (11, st)):
            assert np.array_equal(feet[t, :, :, col], want.astype(np.float32)), (t, col)
    counts = (int(feet[..., 7].sum()), int(feet[..., 8].sum()), int(done.sum()))
    print("touchdowns %d, liftoffs %d, resets %d" % counts)
    assert counts[0] >= 20 and counts[1] >= 20 and counts[2] >= 5
    assert feet[..., 10].max() > 0 and feet[..., 11].max() > 0


def test_a_read_that_does_not_advance_writes_nothing(fix):
    sim, sensor = _loaded(fix, np.arange(200, 264))
    sensor.read(advance=True)
    sensor.read(advance=True)
    before = sensor.state()
    _, feet = _read(sensor)
    assert np.array_equal(sensor.state(), before)
    assert not feet[..., 7:9].any() and np.array_equal(feet[..., 9], np.full((64, 4), np.float32(2) * np.float32(0.008)))
    f_host, feet_host = sensor.read_host()                                      # the host form: the same rows, no advance either
    assert np.array_equal(feet_host, feet) and np.array_equal(sensor.state(), before) and f_host.shape == (64, 13, 3)
    sensor.reset(np.arange(64) % 2)                                             # the named envs start over at the next advancing read
    sensor.read(advance=True)
    _, feet = _read(sensor)
    assert np.array_equal(feet[..., 9], np.where(np.arange(64) % 2, 1, 3)[:, None].repeat(4, 1).astype(np.float32) * np.float32(0.008))
    sensor.close(), sim.close()


def test_state_replays_the_rest_of_the_run(walk):
    run, acts = _Run(), _actions()
    run.sim.restore(walk["mid"][1])
    run.sensor.load_state(walk["mid"][0])
    for t in range(40, T_WALK):
        run.step(acts[t])
        assert np.array_equal(run.bits(), walk["bits"][t]), t
    assert np.array_equal(run.sensor.state(), walk["end"])
    with pytest.raises(ValueError):
        run.sensor.load_state(walk["end"][:-4])
    run.close()


def test_env_snapshot_carries_the_sensor():
    from quadruped_gym_amd.envs.walking import WalkingQuadrupedVecEnv
    n = 33
    acts = torch.tensor(np.random.default_rng(5).uniform(-1, 1, (30, n, 12)).astype(np.float32)).to(DEV)

    def make():
        env = WalkingQuadrupedVecEnv(n, max_time=0.1, device_commands=True, random_controls=True)
        sensor = env.contact_sensor(1.0)
        assert env.contact_sensor(1.0) is sensor
        env.reset()
        return env, sensor, [torch.zeros(s, device=DEV) for s in ((n, 33), (n,))] + [torch.zeros(n, device=DEV, dtype=torch.uint8)]

    def run(env, sensor, bufs, lo, hi):
        out = []
        for t in range(lo, hi):
            env.step_tensor(acts[t], *bufs)
            force, feet = sensor.read(done=bufs[2])
            torch.cuda.synchronize()
            out.append(np.concatenate([x.cpu().numpy().astype(np.float32).view(np.uint32).ravel() for x in (bufs[0], force, feet)]))
        return out

    env, sensor, bufs = make()
    run(env, sensor, bufs, 0, 12)
    snap = env.snapshot()
    assert "contact" in snap
    want = run(env, sensor, bufs, 12, 30)
    env.reset()                                                                 # the env's reset restarts the timers
    _, feet = sensor.read()
    torch.cuda.synchronize()
    assert (feet[..., 9].cpu().numpy() == np.float32(0.008)).all() and not feet[..., 10:].any()
    env2, sensor2, bufs2 = make()
    env2.restore(snap)
    got = run(env2, sensor2, bufs2, 12, 30)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    with pytest.raises(ValueError):
        env2.restore({k: v for k, v in snap.items() if k != "contact"})
    with pytest.raises(ValueError):
        env2.contact_sensor(2.0)
    env.close(), env2.close()
    assert sensor._h is None and sensor2._h is None                             # closed with the env


def test_graph_replay_is_the_eager_run(walk):
    """One env-step and the read behind it, captured once and replayed 16 times: the bits of 16 eager steps, timers included."""
    run, acts = _Run(), _actions()
    fresh, sim0 = run.sensor.state(), run.sim.snapshot()
    s_act = torch.zeros((N_WALK, 12), device=DEV)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run.sim.step_device_packed(s_act, run.packed, stream=side)
        run.sensor.read(done=run.packed[:, 34], body_force=run.force, feet=run.feet, stream=side)
    run.sim.restore(sim0)                                                       # whatever a capture may have run, start from the fresh state
    run.sensor.load_state(fresh)
    timers = R.Timers(N_WALK)
    for t in range(16):
        s_act.copy_(acts[t])
        torch.cuda.synchronize()
        graph.replay()
        assert np.array_equal(run.bits(), walk["bits"][t]), t
        timers.advance(walk["feet"][t, :, :, 6] > 0.5, walk["done"][t])
    blob = run.sensor.state()
    want = np.concatenate([np.stack([timers.prev, timers.phase, timers.last_air, timers.last_stance], -1).ravel(), timers.armed])
    assert np.array_equal(np.frombuffer(blob.tobytes()[24:], np.int32), want)
    del graph
    run.close()


# ---- 3. refusals and the facade ------------------------------------------------------------------------------------------------------------
def test_bad_tensors_raise_before_any_launch(fix):
    sim, sensor = _loaded(fix, np.arange(8))
    good_f, good_feet = torch.zeros((8, 13, 3), device=DEV), torch.zeros((8, 4, 12), device=DEV)
    before = sensor.state()
    bad = [dict(body_force=good_f.double()), dict(body_force=torch.zeros((8, 39), device=DEV)), dict(body_force=good_f.cpu()),
           dict(body_force=torch.zeros((8, 3, 13), device=DEV).transpose(1, 2)), dict(feet=good_feet.half()),
           dict(feet=torch.zeros((9, 4, 12), device=DEV)), dict(feet=torch.zeros(8 * 48 + 1, device=DEV)[1:].view(8, 4, 12)),
           dict(done=torch.zeros(8, device=DEV, dtype=torch.int32)), dict(done=torch.zeros(7, device=DEV)), dict(done=torch.zeros(8))]
    for kw in bad:
        with pytest.raises(ValueError):
            sensor.read(**kw)
    assert np.array_equal(sensor.state(), before)                               # nothing advanced
    for done in (torch.zeros(8, device=DEV, dtype=torch.bool), torch.zeros(8, device=DEV), torch.zeros((8, 35), device=DEV)[:, 34]):
        sensor.read(done=done)
    lib = _abi.load_library()
    assert lib.qg_contact_read_device(sensor._h, None, 0, 1, 1, None, None, None) == -1 and b"both NULL" in lib.qg_last_error()
    assert lib.qg_contact_read_device(sensor._h, good_f.data_ptr(), 2, 1, 1, good_f.data_ptr(), None, None) == -1
    assert lib.qg_contact_read_device(sensor._h, good_f.data_ptr(), 0, 0, 1, good_f.data_ptr(), None, None) == -1
    force_only = np.zeros((8, 13, 3), np.float32)                               # one output is enough
    assert lib.qg_contact_read(sensor._h, force_only.ctypes.data, None) == 0 and force_only.any()
    sensor.close(), sim.close()


def test_refused_in_resident_mode_and_invisible_to_the_simulator():
    n = 64
    a, b = BatchedSim(n, task=_walk_task()), BatchedSim(n, task=_walk_task())
    a.reset(seed=2), b.reset(seed=2)
    sensor = ContactSensor(a)
    mail_a, mail_p = torch.zeros((2, n, 12), device=DEV), torch.zeros((2, n, 35), device=DEV)
    a.resident_start(mail_a, mail_p)
    with pytest.raises(_abi.QuadGymError, match="qg_resident_stop first"):
        sensor.read()
    with pytest.raises(_abi.QuadGymError, match="qg_resident_stop first"):
        sensor.read_host()
    a.resident_stop()
    force, feet = sensor.read()
    torch.cuda.synchronize()
    assert torch.isfinite(force).all() and torch.isfinite(feet).all()
    sensor.close()
    # a sensor created, read and closed leaves the simulator's rollout as an untouched twin's
    acts = torch.tensor(np.random.default_rng(9).uniform(-1, 1, (12, n, 12)).astype(np.float32)).to(DEV)
    pa, pb = torch.zeros((n, 35), device=DEV), torch.zeros((n, 35), device=DEV)
    for t in range(12):
        a.step_device_packed(acts[t], pa), b.step_device_packed(acts[t], pb)
        torch.cuda.synchronize()
        assert torch.equal(pa, pb), t
    for x, y in zip(a.get_state(), b.get_state()):
        assert np.array_equal(x, y)
    a.close(), b.close()


def test_facade_reports_the_weight_of_a_standing_robot(oracle):
    from quadruped_gym_amd.envs.quadruped import QuadrupedEnv
    env = QuadrupedEnv(model_path="builtin")
    env.reset()
    assert env._contact is None                                                 # nothing is created until the fields are read
    for _ in range(150):                                                        # 1.2 s: the robot settles on its feet
        env.step(np.array([0, 0, -0.5] * 4))
    assert env._contact is None
    force, flags = env.data.contact_force, env.data.foot_contact
    assert force.shape == (13, 3) and force.dtype == np.float64 and flags.shape == (4,) and flags.dtype == bool
    model = oracle.default_model()
    want = R.evaluate(model, env.data.qpos[None], env.data.qvel[None])
    weight = -model.gravity[2] * sum(model.body_mass[b] for b in range(13))
    # the oracle's own sum at that state differs from the weight by the robot's residual acceleration: that is the tolerance
    tol = abs(want["force"][0, :, 2].sum() - weight) + R.tolerance(R.BUDGET_FORCE_NORMAL, want["force"][0, :, 2], R.MARGIN).sum()
    print("sum F_z %.4f N, weight %.4f N, oracle's sum %.4f N, tolerance %.4f N" % (force[:, 2].sum(), weight, want["force"][0, :, 2].sum(), tol))
    assert abs(force[:, 2].sum() - weight) <= tol and tol < 0.05 * weight
    band = R.flag_band(want)[0, FEET]
    assert np.array_equal(flags[~band], R.flags(want["force"])[0, FEET][~band]) and flags.any()
    env.data.qpos[2] += 0.5                                                     # an edit of data is seen: the robot is in the air
    assert not env.data.foot_contact.any() and not env.data.contact_force.any()
    env.close()
    assert env._contact is None
