"""The privileged state's definition (tests/privileged_reference.py) pinned without a GPU: the gravity direction is a unit vector, the
dynamics columns default to the identity row, the push schedule's restatement in integers agrees with the oracle's counter hash and
with hand-worked windows, and the float32 budget of the two rotated columns is MEASURED here -- over the states of
golden/contact_cells.npz and a seeded pool of tilted bases at up to 2 m/s -- and held against the module's BUDGET_* pairs."""
import numpy as np
import pytest

import contact_cells as CC
import contact_sensor_reference as CR
import privileged_reference as P

from quadruped_gym_amd import _abi

# The keys.  tests/test_external_wrench_checker.py pins the wrench checker and the layout of qg_push_params; it holds no push key (no
# seed, env, episode or schedule) to restate.  The keys the suite does check the schedule with are those of the push test of
# tests/test_external_wrench_gpu.py -- this schedule, seed 21, episodes 1 and 2 -- so they are restated here (nothing is imported):
# the GPU and the CPU then pin the same windows.
PUSH = {"interval": 3, "duration": 2, "probability": 0.6, "force": (4.0, 12.0)}
SEED = 21


@pytest.fixture(scope="module")
def states():
    fix = CC.load()
    pq, pv = P.pool()
    return np.concatenate([fix["qpos"], pq]), np.concatenate([fix["qvel"], pv])


def test_gravity_direction_is_a_unit_vector_and_level_is_down(states):
    _, g = P.base_columns(*states)
    assert np.abs(np.linalg.norm(g, axis=1) - 1.0).max() < 1e-12
    q = np.zeros((1, 19))
    q[0, 3] = 2.0                                       # identity orientation, not normalised
    lin, g = P.base_columns(q, np.array([[0.3, -0.2, 0.1] + [0.0] * 15]))
    assert np.array_equal(g, [[0.0, 0.0, -1.0]]) and np.allclose(lin, [[0.3, -0.2, 0.1]], atol=0, rtol=1e-15)
    # a quarter turn about z: the world's x velocity is the body's -y
    q[0, 3:7] = [np.sqrt(0.5), 0, 0, np.sqrt(0.5)]
    lin, _ = P.base_columns(q, np.array([[1.0] + [0.0] * 17]))
    assert np.allclose(lin, [[0.0, -1.0, 0.0]], atol=1e-15)


def test_columns_and_identity_row(oracle):
    model = oracle.default_model()
    assert P.COLUMNS == _abi.PRIV_COLUMNS and P.DIM == _abi.PRIV_DIM == 85
    first = 0
    for _, lo, width in P.COLUMNS:                      # the table tiles the 85 columns
        assert lo == first
        first += width
    assert first == P.DIM
    fix = CC.load()
    k = slice(0, 9)
    out, ref = P.evaluate(model, fix["qpos"][k], fix["qvel"][k], fix["act"][k], fix["nstep"][k])
    row = out[:, P.COL["dynamics"]]
    assert np.array_equal(row, np.tile(_abi.identity_dynamics_row(_abi.default_model()), (9, 1)))
    assert np.array_equal(row[0], [np.float32(model.contact_friction), 0, 0, 0, 0, 1, 1, 1, 1, 1, 1])
    assert not out[:, P.COL["frame_wrench"]].any()
    assert np.array_equal(out[:, P.COL["foot_force"]].reshape(9, 4, 3), ref["force"][:, list(CR.FEET)])
    assert np.array_equal(out[:, P.COL["episode_time"]][:, 0], fix["nstep"][k].astype(np.float32) * np.float32(model.timestep))
    assert np.array_equal(out[:, P.COL["body_contact"]][:, 0], (ref["force"][:, P.NON_FOOT, 2] > 0).sum(1))


def test_push_hash_is_the_oracles(oracle):
    L = oracle.lib()
    for env in (0, 5, 4097):
        for episode in (1, 2):
            for stream in (32, 33, 34, 35, 36, 43):
                assert P.bits24(SEED, env, episode, stream) == int(round(L.qgo_uniform_stream(SEED, env, episode, stream) * 2.0 ** 24))


def test_push_windows_by_hand():
    """Every window of the first 30 env-steps of 12 keys, worked from the four integers of the window."""
    held = []
    for env in range(6):
        for episode in (1, 2):
            for w in range(10):
                st = 32 + 4 * w
                k = [P.bits24(SEED, env, episode, st + c) for c in range(4)]
                forces = [P.push_force(PUSH, SEED, env, episode, 3 * w + j) for j in range(3)]
                if not k[0] < 0.6 * 2 ** 24:              # (0.6 as an f32 is 10066330 / 2^24: the gate is k < 10066330)
                    assert k[0] >= 10066330 and forces == [(0.0, 0.0)] * 3
                    continue
                assert k[0] < 10066330
                o = (k[1] * 2) >> 24                    # interval - duration + 1 = 2: the push starts at offset 0 or 1
                assert o == (1 if k[1] >= 2 ** 23 else 0)
                F, th = 4.0 + 8.0 * k[2] / 2 ** 24, 2 * np.pi * k[3] / 2 ** 24
                for j in range(3):
                    want = (F * np.cos(th), F * np.sin(th)) if o <= j < o + 2 else (0.0, 0.0)
                    assert np.allclose(forces[j], want, rtol=1e-14, atol=0)
                    held.append(want != (0.0, 0.0))
                assert 4.0 <= np.hypot(*forces[o]) <= 12.0 + 1e-12
    assert 0.3 < np.mean(held) < 0.9
    # the float32 form is the float64 one within the bound the GPU test uses; no schedule, no force
    for s in range(30):
        f64, f32 = P.push_force(PUSH, SEED, 3, 1, s), P.push_force(PUSH, SEED, 3, 1, s, np.float32)
        assert np.abs(np.array(f32, np.float64) - f64).max() <= P.PUSH_RTOL * 12.0
        assert (f64 == (0.0, 0.0)) == (f32 == (0.0, 0.0))
    assert P.push_force(None, SEED, 0, 1, 0) == (0.0, 0.0)
    # two episodes of an env draw different pushes
    a = [P.push_force(PUSH, SEED, 0, 1, s) for s in range(30)]
    assert a != [P.push_force(PUSH, SEED, 0, 2, s) for s in range(30)]


def test_float32_budget_of_the_rotated_columns(states):
    """The measurement the module's BUDGET_* pairs come from: printed, and held against them (a share above 1 fails; one below 0.25
    means the pair no longer describes the arithmetic and should be measured again)."""
    assert np.abs(states[1][:, :3]).max() > 1.9 and len(states[0]) == 664 + P.POOL_SIZE
    lin64, g64 = P.base_columns(*states)
    lin32, g32 = P.base_columns(*states, dtype=np.float32)
    assert lin32.dtype == np.float32 and g32.dtype == np.float32
    for name, got, want, budget in (("gravity_dir", g32, g64, P.BUDGET_GRAVITY_DIR), ("base_lin_vel", lin32, lin64, P.BUDGET_BASE_LIN_VEL)):
        err = got.astype(np.float64) - want
        share = CR.share(err, budget, want)
        print("%s: largest |f32 - f64| %.3e, largest share of (%.1e + %.1e |f64|): %.3f" % (name, np.abs(err).max(), *budget, share))
        assert 0.25 < share <= 1.0, (name, share)
