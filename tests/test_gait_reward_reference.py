"""The gait reward's definition (tests/gait_reward_reference.py) without a GPU: every term on hand-computed rows -- a finished env, a
non-advancing read, the gate on either side of and exactly at min_command_speed --, the float32 evaluation in the stated order inside
the stated budget over the fixture's 664 states (printed: this is where the GPU test's tolerance comes from), and what the fixture
reaches with the shared parameters."""
import numpy as np
import pytest

import contact_cells as CC
import contact_sensor_reference as S
import gait_reward_reference as G

P = dict(G.PARAMS, force_threshold=G.FORCE_THRESHOLD)


@pytest.fixture(scope="module")
def rows(oracle):
    fix = CC.load()
    return G.fixture_rows(S.evaluate(oracle.default_model(), fix["qpos"], fix["qvel"]))


def _foot(z=0.0, vx=0.0, vy=0.0, vz=0.0, contact=0, touchdown=0, air=0.0):
    r = np.zeros(12, np.float32)
    r[G.POS_Z], r[G.VEL_X], r[G.VEL_Y], r[G.VEL_Z], r[G.CONTACT], r[G.TOUCHDOWN], r[G.LAST_AIR_TIME] = z, vx, vy, vz, contact, touchdown, air
    return r


def _env(feet, fz):
    force = np.zeros((13, 3), np.float32)
    force[:, 2] = fz
    return force, np.stack(feet)


def test_terms_on_hand_computed_rows():
    unit = dict(P, weights={name: 1.0 for name in G.TERMS}, air_time_target=0.02, clearance_target=0.05, max_contact_force=20.0)
    fz = np.zeros(13, np.float32)
    fz[3], fz[6], fz[0], fz[1], fz[2] = 25.0, 21.5, 1.5, 1.0, 0.5           # two feet over 20 N; FRAME over the 1 N threshold, body 1 ON it
    feet = [_foot(vx=0.5, vy=0.25, vz=-2.0, contact=1, touchdown=1, air=0.032),   # touches down after 4 steps, sliding
            _foot(vx=1.0, contact=1),                                             # stands, sliding
            _foot(z=0.25, vx=3.0, vy=4.0),                                        # swings 0.2 m above the target at 5 m/s
            _foot(z=0.05, vx=1.0, touchdown=1, air=0.5)]                          # inconsistent row: touchdown without contact still counts
    force, rows = _env(feet, fz)
    out = G.evaluate(force[None], rows[None], **unit)
    want = [(0.032 - 0.02) + (0.5 - 0.02), (0.25 + 0.0625) + 1.0, 0.2 ** 2 * 5.0 + 0.0, 4.0 + 0.0, 5.0 + 1.5, 1.0, 0.0]
    assert np.allclose(out["terms"][0], want, rtol=1e-6, atol=1e-9), (out["terms"][0], want)
    assert out["terms"][0, 5] == 1.0 and out["terms"][0, 6] == 0.0          # Fz == threshold is not contact
    assert np.allclose(out["shaped"][0], sum(want), rtol=1e-6) and np.array_equal(out["reward_out"], out["shaped"])
    # weights and the reward
    w = dict(G.WEIGHTS)
    got = G.evaluate(force[None], rows[None], reward=np.array([1.5], np.float32), **dict(unit, weights=w))
    wv = [w[name] for name in G.TERMS]
    assert np.allclose(got["components"][0], np.array(wv) * want, rtol=1e-6, atol=1e-9)
    assert np.allclose(got["reward_out"][0], 1.5 + float(np.dot(wv, want)), rtol=1e-6)
    # nobody on the ground: flight
    air = G.evaluate(np.zeros((1, 13, 3), np.float32), np.stack([_foot(z=0.05)] * 4)[None], **unit)
    assert air["terms"][0].tolist() == [0, 0, 0, 0, 0, 0, 1]


def test_finished_env_non_advancing_read_and_the_gate():
    fz = np.zeros(13, np.float32)
    fz[3] = 30.0
    force, rows = _env([_foot(vx=1.0, vz=1.0, contact=1, touchdown=1, air=0.1)] + [_foot(z=0.3, vx=1.0)] * 3, fz)
    force, rows = np.stack([force] * 4), np.stack([rows] * 4)
    reward = np.array([0.1, 0.2, 0.3, 0.4], np.float32)
    base = np.arange(8, dtype=np.float32).reshape(4, 2)
    limit = np.float32(G.MIN_COMMAND_SPEED)
    command = np.array([[limit, -limit], [np.nextafter(limit, np.float32(1)), 0], [0, -np.nextafter(limit, np.float32(1))], [0.05, 0.0]], np.float32)
    for dtype in (np.float64, np.float32):
        out = G.evaluate(force, rows, done=np.array([0, 1, 0, 0]), command=command, reward=reward, base=base, dtype=dtype, **P)
        # a finished env: seven exact zeros, the reward bit for bit
        assert not out["components"][1].any() and out["reward_out"][1] == reward[1] and out["terms"][1].any()
        # the gate: max-norm strictly above min_command_speed; exactly at it is closed
        assert out["terms"][0, 0] == 0 and out["terms"][3, 0] == 0 and out["terms"][2, 0] != 0
        assert out["terms"][2, 0] == dtype(np.float32(0.1)) - dtype(np.float32(G.AIR_TIME_TARGET))
        assert np.array_equal(out["terms"][:, 1:], np.broadcast_to(out["terms"][0, 1:], (4, 6)))     # the gate touches term 0 alone
        assert out["wide"].shape == (4, 9) and np.array_equal(out["wide"][:, :2], base) and np.array_equal(out["wide"][:, 2:], out["components"])
        assert out["reward_out"].dtype == dtype
    # no command: the gate is open
    assert G.evaluate(force, rows, **P)["terms"][0, 0] != 0
    # a non-advancing read shows no touchdown: terms 0 and 3 are zero, the others stay
    quiet = rows.copy()
    quiet[..., G.TOUCHDOWN] = 0
    a, b = G.evaluate(force, quiet, **P)["terms"], G.evaluate(force, rows, **P)["terms"]
    assert not a[:, [0, 3]].any() and b[:, [0, 3]].all() and np.array_equal(a[:, [1, 2, 4, 5, 6]], b[:, [1, 2, 4, 5, 6]])


def test_float32_evaluation_is_inside_the_budget(rows):
    force, feet = rows
    done, command, reward, base = G.fixture_extras(len(feet))
    e64 = G.evaluate(force, feet, done, command, reward, base, **P)
    e32 = G.evaluate(force, feet, done, command, reward, base, dtype=np.float32, **P)
    assert e32["components"].dtype == np.float32 and e32["reward_out"].dtype == np.float32
    shares = {}
    for k, name in enumerate(G.TERMS):
        err = np.abs(e32["terms"][:, k].astype(np.float64) - e64["terms"][:, k])
        tol = G.term_tolerance(e64["terms"])[:, k]
        j = int(err.argmax())
        shares[name] = float(np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0)).max())
        print("%-19s largest |f32 - f64| %.3e (where f64 = %.5g); largest share of atol %.1e + rtol %.1e |f64|: %.3f"
              % (name, err.max(), e64["terms"][j, k], *G.BUDGET_TERM[name], shares[name]))
    assert all(s <= 1.0 for s in shares.values()), shares
    # the budget is a measurement rounded up, not a free parameter: within a factor 3 of what is measured (the two integer terms: exact)
    assert all(shares[name] >= 1.0 / 3.0 for name in G.TERMS[:5]), shares
    assert shares["body_contact"] == 0.0 and shares["flight"] == 0.0
    for what, got, want, tol in (("components", e32["components"], e64["components"], G.component_tolerance(e64, G.WEIGHTS)),
                                 ("reward_out", e32["reward_out"], e64["reward_out"], G.reward_tolerance(e64, G.WEIGHTS, reward))):
        err = np.abs(got.astype(np.float64) - want)
        ok = tol > 0
        print("%-19s largest |f32 - f64| %.3e; largest share of its bound %.3f" % (what, err.max(), float((err[ok] / tol[ok]).max())))
        assert (err <= tol).all()
    assert not e32["components"][done].any() and np.array_equal(e32["reward_out"][done], reward[done])
    assert np.array_equal(e32["wide"][:, :11], base)


def test_census_of_what_the_fixture_reaches(rows):
    force, feet = rows
    t = G.evaluate(force, feet, **P)["terms"]
    fz = force[..., 2]
    foot_contacts = int((fz[:, list(G.FEET)] > 1.0).sum())
    counts = dict(slip=int((t[:, 1] != 0).sum()), clearance=int((t[:, 2] != 0).sum()), contact_force=int((t[:, 4] != 0).sum()),
                  body_contact=int((t[:, 5] >= 1).sum()), flight=int((t[:, 6] == 1).sum()), grounded=int((t[:, 6] == 0).sum()),
                  air_time_positive=int((t[:, 0] > 0).sum()), air_time_negative=int((t[:, 0] < 0).sum()), touchdown_speed=int((t[:, 3] != 0).sum()))
    print("664 states: %d foot contacts above 1 N, %d foot forces above 20 N;" % (foot_contacts, int((fz[:, list(G.FEET)] > 20.0).sum())), counts)
    assert len(t) == 664
    assert counts["slip"] >= 150 and counts["clearance"] >= 400 and counts["contact_force"] >= 40
    assert counts["body_contact"] >= 400 and counts["flight"] >= 400 and counts["grounded"] >= 150
    assert counts["air_time_positive"] >= 20 and counts["air_time_negative"] >= 20 and counts["touchdown_speed"] >= 40    # the synthetic events
    assert set(np.unique(t[:, 5])) <= set(range(10)) and t[:, 5].max() >= 3


def test_names_and_shared_parameters():
    assert G.TERMS == ("feet_air_time", "feet_slip", "feet_clearance", "touchdown_speed", "feet_contact_force", "body_contact", "flight")
    assert set(G.WEIGHTS) == set(G.TERMS) and all(w != 0 for w in G.WEIGHTS.values())
    assert any(w > 0 for w in G.WEIGHTS.values()) and any(w < 0 for w in G.WEIGHTS.values())
    assert (G.FORCE_THRESHOLD, G.MAX_CONTACT_FORCE, G.CLEARANCE_TARGET) == (1.0, 20.0, 0.05)
    assert G.AIR_TIME_TARGET == (G.AIR_TIME_K + 0.5) * G.DT and isinstance(G.AIR_TIME_K, int)
    assert G.FEET == S.FEET and len(G.NON_FEET) == 9 and (G.N_WALK, G.T_WALK) == (67, 80)
    assert G.walk_actions().shape == (80, 67, 12)
