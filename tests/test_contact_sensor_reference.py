"""The contact sensor's definition (tests/contact_sensor_reference.py) without a GPU: the restated forces are the oracle's, the foot
velocities are the derivative of the oracle's kinematics, the float32 evaluation stays inside the stated budget (printed: this is where
the GPU test's tolerance comes from), the fixture reaches what the GPU test relies on, and the integer timers give hand-written answers."""
import numpy as np
import pytest

import contact_cells as CC
import contact_sensor_reference as R


@pytest.fixture(scope="module")
def fix():
    return CC.load()


@pytest.fixture(scope="module")
def ref(oracle, fix):
    return R.evaluate(oracle.default_model(), fix["qpos"], fix["qvel"])


@pytest.fixture(scope="module")
def diag(oracle, fix):
    """(contact_F [n, 13, 3], contact_W [n, 13]) of the oracle's first substep from every fixture state."""
    model, n = oracle.default_model(), len(fix["qpos"])
    F, W = np.zeros((n, 13, 3)), np.zeros((n, 13))
    for i in range(n):
        e = oracle.make_env(fix["qpos"][i], fix["qvel"][i], fix["act"][i])
        _, dg = oracle.substep(model, e, np.zeros(12), want_diag=True)
        F[i], W[i] = [list(r) for r in dg.contact_F], list(dg.contact_W)
    return F, W


def test_restated_forces_are_the_oracles(fix, ref, diag):
    F, W = diag
    assert len(fix["qpos"]) == 664
    err = float(np.abs(ref["force"] - F).max())
    print("restated force against the oracle's contact_F: %.3g N" % err)
    assert err <= 1e-9
    assert np.array_equal(W > 0, ref["under"].any(2))
    assert np.array_equal(W > 0, ref["W"] > 0)


def test_foot_velocities_are_the_derivative_of_the_kinematics(oracle, fix, ref):
    model = oracle.default_model()
    placer = CC.Placer(oracle, model)
    placer.cps = [np.zeros((1, 3))] * CC.NBODY                # point 0 of every body: its frame origin
    worst, worst_pos = 0.0, 0.0
    for e in range(len(fix["qpos"])):
        q, v = fix["qpos"][e].astype(np.float64), fix["qvel"][e].astype(np.float64)
        xpos, _, _ = oracle.kinematics(model, q)
        for f, b in enumerate(R.FEET):
            worst = max(worst, float(np.abs(placer.point_velocity(q, v, b, 0) - ref["foot_vel"][e, f]).max()))
            worst_pos = max(worst_pos, float(np.abs(xpos[b] - ref["foot_pos"][e, f]).max()))
    print("foot velocity against the central difference of oracle.kinematics: %.3g m/s; position: %.3g m" % (worst, worst_pos))
    assert worst <= 1e-8 and worst_pos <= 1e-12


def test_float32_evaluation_is_inside_the_budget(oracle, fix, ref):
    e32 = R.evaluate(oracle.default_model(), fix["qpos"], fix["qvel"], dtype=np.float32)
    assert e32["force"].dtype == np.float32 and e32["foot_vel"].dtype == np.float32
    cases = (("force normal", e32["force"][..., 2], ref["force"][..., 2], R.BUDGET_FORCE_NORMAL),
             ("force tangential", e32["force"][..., :2], ref["force"][..., :2], R.BUDGET_FORCE_TANGENTIAL),
             ("foot position", e32["foot_pos"], ref["foot_pos"], R.BUDGET_FOOT_POS),
             ("foot velocity", e32["foot_vel"], ref["foot_vel"], R.BUDGET_FOOT_VEL))
    shares = {}
    for name, got, want, budget in cases:
        err = got.astype(np.float64) - want
        k = np.unravel_index(np.abs(err).argmax(), err.shape)
        shares[name] = R.share(err, budget, want)
        print("%-17s largest |f32 - f64| %.3e (where f64 = %.4g); largest share of atol %.1e + rtol %.1e |f64|: %.3f"
              % (name, np.abs(err).max(), want[k], budget[0], budget[1], shares[name]))
    assert all(s <= 1.0 for s in shares.values()), shares
    # the budget is a measurement rounded up, not a free parameter: it is within a factor 3 of what is measured
    assert all(s >= 1.0 / 3.0 for s in shares.values()), shares
    # flags: equal outside the band
    band = R.flag_band(ref)
    assert not ((R.flags(e32["force"]) != R.flags(ref["force"])) & ~band).any()


def test_census_of_what_the_fixture_reaches(ref):
    fz = ref["force"][..., 2]
    touching = ref["W"] > 0
    per_body = (fz > 0).sum(0)
    clipped = int((touching & (fz == 0)).sum())
    foot_states = int((fz[:, list(R.FEET)] > 0).any(1).sum())
    print("states with F_z > 0 per body:", per_body.tolist(), "; no-adhesion clips: %d of %d touching pairs; states with a foot in contact: %d"
          % (clipped, int(touching.sum()), foot_states))
    assert per_body.min() >= 50
    assert clipped >= 200
    assert foot_states >= 200


@pytest.mark.parametrize("threshold", [0.0, 5.0])
def test_exclusion_band_is_small(ref, threshold):
    band = R.flag_band(ref, threshold)
    assert band.shape == (664, 13) and band.size == 8632
    near_margin = int((ref["gap"] < R.MARGIN_BAND).sum())
    print("threshold %.1f N: %d of %d pairs left out (%d with a point within %.0e m of the margin)"
          % (threshold, int(band.sum()), band.size, near_margin, R.MARGIN_BAND))
    assert band.sum() <= R.MAX_EXCLUDED * band.size
    if threshold == 0.0:
        assert near_margin == 4
        f0, touching = ref["normal_unclipped"], ref["W"] > 0
        assert [int((touching & (np.abs(f0) < t)).sum()) for t in (0.01, 0.05, 0.2)] == [0, 2, 13]


def test_timers_on_a_scripted_table():
    """One env.  Rows: (contact of the four feet, done) -> expected (touchdown, liftoff, phase, last_air, last_stance) per foot.
    Foot 0 walks: air, touchdown, stance, liftoff; foot 1 stands through a done; foot 2 flips at every sample (two transitions in a
    row); foot 3 never touches."""
    c = lambda s: [int(ch) for ch in s]
    script = [
        # contact  done   touchdown liftoff   phase          last_air       last_stance
        ("0100", 0, "0000", "0000", (1, 1, 1, 1), (0, 0, 0, 0), (0, 0, 0, 0)),      # unarmed first sample: no event, whatever prev held
        ("0110", 0, "0010", "0000", (2, 2, 1, 2), (0, 0, 1, 0), (0, 0, 0, 0)),
        ("1100", 0, "1000", "0010", (1, 3, 1, 3), (2, 0, 1, 0), (0, 0, 1, 0)),      # foot 0 touches down after 2 steps in the air
        ("1110", 0, "0010", "0000", (2, 4, 1, 4), (2, 0, 1, 0), (0, 0, 1, 0)),
        ("1100", 1, "0000", "0000", (1, 1, 1, 1), (0, 0, 0, 0), (0, 0, 0, 0)),      # done in mid-stance: everything restarts, no liftoff
        ("1100", 0, "0000", "0000", (2, 2, 2, 2), (0, 0, 0, 0), (0, 0, 0, 0)),
        ("0100", 0, "0000", "1000", (1, 3, 3, 3), (0, 0, 0, 0), (2, 0, 0, 0)),      # liftoff after 2 steps of stance
        ("1100", 0, "1000", "0000", (1, 4, 4, 4), (1, 0, 0, 0), (2, 0, 0, 0)),      # ... and straight down again
    ]
    t = R.Timers(1)
    t.prev[:] = 1                                             # stale: the unarmed sample must not read it
    for k, (contact, done, td, lo, phase, air, stance) in enumerate(script):
        got_td, got_lo = t.advance(np.array([c(contact)]), np.array([done]))
        assert got_td[0].astype(int).tolist() == c(td) and got_lo[0].astype(int).tolist() == c(lo), k
        assert (tuple(t.phase[0]), tuple(t.last_air[0]), tuple(t.last_stance[0])) == (phase, air, stance), k
        assert t.prev[0].tolist() == c(contact) and t.armed[0] == 1
    ph, air, st = t.times(0.008)
    assert ph.dtype == np.float32 and ph[0, 1] == np.float32(4) * np.float32(0.008) and air[0, 0] == np.float32(0.008)
    t.reset(np.array([1]))
    assert t.armed[0] == 0
    td, lo = t.advance(np.array([c("0000")]))
    assert not td.any() and not lo.any() and tuple(t.phase[0]) == (1, 1, 1, 1) and not t.last_stance.any()
