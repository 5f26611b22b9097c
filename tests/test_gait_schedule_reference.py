"""The gait schedule's definition (tests/gait_schedule_reference.py) without a GPU: the hard schedule's measure over a whole period,
kappa = 0, continuity across the wrap, the presets against the model's geometry, the census of the gait draw, the float32 evaluation in
the stated order inside the stated budget over the GPU tests' own inputs (printed: this is where their tolerance comes from), and the
census of the four (scheduled, sensed) cells the fixture states give every foot."""
import numpy as np
import pytest

import contact_cells as CC
import contact_sensor_reference as S
import gait_schedule_reference as R

from quadruped_gym_amd import _abi
from quadruped_gym_amd.model.loader import load_model

from helpers import reference_model


def test_hard_schedule_is_on_for_exactly_D_of_a_period():
    """q -> hard is the indicator of [0, D): over the 2^32 phases it is on for D of them.  Counted exactly from the two edges, and
    checked on a grid that straddles both."""
    off, D = R.table_ints()
    for g, (offsets, duty) in enumerate(R.TABLE):
        assert D[g] == int(np.rint(np.float64(np.float32(duty)) * 2.0 ** 32)) and 0 < D[g] < 2 ** 32
        for f in range(4):
            # hard_f(phi) = (phi + off_f mod 2^32) < D: the set of phi is the interval [-off_f, D - off_f) mod 2^32, of D phases
            edges = np.array([(-int(off[g, f])) % 2 ** 32, (int(D[g]) - int(off[g, f])) % 2 ** 32], np.uint64)
            near = ((edges[:, None].astype(np.int64) + np.arange(-3, 4)[None]) % 2 ** 32).astype(np.uint64)
            hard = R.foot_quantities(near.ravel(), np.full(14, g), dtype=np.float64)[0][:, f].reshape(2, 7)
            assert hard[0].tolist() == [False] * 3 + [True] * 4 and hard[1].tolist() == [True] * 3 + [False] * 4, (g, f)
    # ... and by count on a coarse grid of a short period: 2^16 phases spaced 2^16 apart see D / 2^16 of them on, to the grid's grain
    grid = (np.arange(2 ** 16, dtype=np.uint64) << np.uint64(16))
    for g in range(len(R.TABLE)):
        hard = R.foot_quantities(grid, np.full(len(grid), g))[0]
        assert (np.abs(hard.sum(0) - float(D[g]) / 2 ** 16) <= 1).all()


def test_kappa_zero_is_the_hard_schedule():
    phi = np.random.default_rng(0).integers(0, 2 ** 32, 4096, dtype=np.uint64)
    for dtype in (np.float64, np.float32):
        for g in range(len(R.TABLE)):
            hard, _, _, s = R.foot_quantities(phi, np.full(len(phi), g), kappa=0.0, dtype=dtype)
            assert np.array_equal(s, hard.astype(dtype))
            _, _, _, soft = R.foot_quantities(phi, np.full(len(phi), g), kappa=R.KAPPA, dtype=dtype)
            assert ((soft > 0.5) <= hard).all() and ((soft < 0.5) <= ~hard).all() and ((soft > 0) & (soft < 1)).any()


def test_s_is_continuous_across_the_wrap_and_both_edges():
    """One phase step of 2^8 (the grain of p) moves s by at most inv2k x 2^-24, at the wrap q = 2^32 - 1 -> 0 and at q = D as anywhere."""
    off, D = R.table_ints()
    step = 2.0 ** -24 / (2.0 * R.KAPPA)
    for g in range(len(R.TABLE)):
        for centre in (0, int(D[g])):
            for grains in (1, 256):                                                 # next to the edge grain by grain; the whole ramp
                q = ((centre + 256 * grains * np.arange(-600, 601)) % 2 ** 32).astype(np.uint64)
                phi = (q - off[g, 0]) & R.M32
                for dtype in (np.float64, np.float32):
                    s = R.foot_quantities(phi, np.full(len(phi), g), dtype=dtype)[3][:, 0].astype(np.float64)
                    assert np.abs(np.diff(s)).max() <= grains * step * 1.0001, (g, centre, dtype)
                    assert abs(s[600] - 0.5) <= step                                # the edge itself
                    if grains == 256:
                        assert {s.min(), s.max()} == {0.0, 1.0}                     # the whole ramp is inside the window


def test_presets_pair_the_legs_the_geometry_says(tmp_path):
    from quadruped_gym_amd.schedule import GAITS, gait_presets, leg_pairs
    qg, _ = load_model(reference_model(tmp_path))                                   # the fixture model's body positions
    hips = np.array([[qg.body_pos[1 + 3 * k][d] for d in range(2)] for k in range(4)])
    assert (np.sign(hips) == [[-1, 1], [-1, -1], [1, -1], [1, 1]]).all()            # legs 1..4 of quadruped.xml
    diagonals, laterals, fore_hind = leg_pairs(hips)
    assert {frozenset(p) for p in diagonals} == {frozenset((0, 2)), frozenset((1, 3))}
    assert {frozenset(p) for p in laterals} == {frozenset((0, 3)), frozenset((1, 2))}
    assert fore_hind == ((2, 3), (0, 1))
    assert gait_presets(hips) == GAITS and set(GAITS) == {"trot", "pace", "bound", "pronk", "walk"}
    for name, (offsets, duty) in GAITS.items():
        assert (tuple(offsets), duty) == R.GAITS[name], name
    same = lambda name, pair: GAITS[name][0][pair[0]] == GAITS[name][0][pair[1]]
    assert all(same("trot", p) for p in diagonals) and not any(same("trot", p) for p in laterals + fore_hind)
    assert all(same("pace", p) for p in laterals) and not any(same("pace", p) for p in diagonals + fore_hind)
    assert all(same("bound", p) for p in fore_hind) and not any(same("bound", p) for p in diagonals + laterals)
    assert len(set(GAITS["pronk"][0])) == 1 and sorted(GAITS["walk"][0]) == [0.0, 0.25, 0.5, 0.75]
    with pytest.raises(ValueError):
        leg_pairs([[1, 1], [1, 2], [-1, 1], [-1, -1]])                              # two hips in one quadrant


def test_gait_draw_reaches_every_table_entry():
    for seed in R.SEEDS:
        for n in R.SIZES[1:]:
            g = np.concatenate([R.draws(seed, np.arange(n), np.full(n, ep))[0] for ep in range(8)])
            assert set(g.tolist()) == set(range(len(R.TABLE))), (seed, n, np.bincount(g, minlength=len(R.TABLE)))
        g, fr, phi0 = R.draws(seed, np.arange(4096), np.zeros(4096, np.int64))
        assert np.bincount(g, minlength=5).min() >= 700 and fr.dtype == np.float32
        assert fr.min() >= np.float32(R.FREQ[0]) and fr.max() <= np.float32(R.FREQ[1]) and fr.max() > 2.9 and fr.min() < 1.1
        assert (phi0 & np.uint64(0xFF) == 0).all() and phi0.max() < 2 ** 32 and len(np.unique(phi0)) > 4000
        assert (R.dphi(fr) <= 2 ** 31).all() and R.dphi(np.float32(3.0)) * R.STEPS > 2 * 2 ** 32          # wraps at least twice
    # a key space of its own: not the perturbation layer's draws
    import perturb_reference as P
    assert not np.array_equal(R.k(0, np.arange(64), 0, 0), P.k_int(0, np.arange(64), 0, 0))


@pytest.fixture(scope="module")
def sensed(oracle):
    """The sensor's float64 rows at the 67 fixture states, rounded to float32 as a launch reports them."""
    fix = CC.load()
    idx = R.fixture_states(fix)
    ref = S.evaluate(oracle.default_model(), fix["qpos"][idx], fix["qvel"][idx])
    feet = np.zeros((len(idx), 4, 12), np.float32)
    feet[..., 0:3], feet[..., 3:6] = ref["foot_pos"], ref["foot_vel"]
    return ref["force"].astype(np.float32), feet


def _phases(seed, n=67):
    """The views of STEPS steps of a checker without finished envs."""
    chk = R.Checker(n, seed=seed, **R.PARAMS)
    return [chk.step()[1] for _ in range(R.STEPS)]


def test_float32_evaluation_is_inside_the_budget(sensed):
    force, feet = sensed
    done, command, reward, base = R.extras(len(feet))
    worst = {name: 0.0 for name in R.TERMS}
    worst_clock = worst_c = worst_r = 0.0
    for seed in R.SEEDS:
        for view in _phases(seed):
            e64 = R.evaluate(view, force, feet, done, command, reward, base, **R.PARAMS)
            e32 = R.evaluate(view, force, feet, done, command, reward, base, dtype=np.float32, **R.PARAMS)
            assert e32["components"].dtype == np.float32 and np.array_equal(e32["hard"], e64["hard"])
            assert np.array_equal(e32["s"].astype(np.float64), e64["s"])            # s_f is exact in float32
            tol = R.term_tolerance(e64["terms"])
            err = np.abs(e32["terms"].astype(np.float64) - e64["terms"])
            for j, name in enumerate(R.TERMS):
                share = np.where(tol[:, j] > 0, err[:, j] / np.where(tol[:, j] > 0, tol[:, j], 1), np.where(err[:, j] > 0, np.inf, 0))
                worst[name] = max(worst[name], float(share.max()))
            tol_c, tol_r = R.component_tolerance(e64), R.reward_tolerance(e64, reward=reward)
            err_c, err_r = np.abs(e32["components"].astype(np.float64) - e64["components"]), np.abs(e32["reward_out"].astype(np.float64) - e64["reward_out"])
            assert (err_c <= tol_c).all() and (err_r <= tol_r).all()
            worst_c = max(worst_c, float((err_c / np.where(tol_c > 0, tol_c, 1)).max()))
            worst_r = max(worst_r, float((err_r / np.where(tol_r > 0, tol_r, 1)).max()))
            assert not e32["components"][done].any() and np.array_equal(e32["reward_out"][done], reward[done])
            c64, c32 = R.columns(view), R.columns(view, dtype=np.float32)
            assert np.array_equal(c32[:, 8:].astype(np.float64), c64[:, 8:])        # freq and d: exact
            worst_clock = max(worst_clock, float(np.abs(c32[:, :8].astype(np.float64) - c64[:, :8]).max()))
    for name in R.TERMS:
        print("%-16s largest share of atol %.1e + rtol %.1e |f64|: %.3f" % (name, *R.BUDGET_TERM[name], worst[name]))
    print("components: largest share of their bound %.3f; reward_out %.3f" % (worst_c, worst_r))
    print("clock columns: E_clock = largest |f32 - f64| %.3e, share of BUDGET_CLOCK %.3f" % (worst_clock, worst_clock / R.BUDGET_CLOCK))
    assert all(share <= 1.0 for share in worst.values()), worst
    # the budget is a measurement rounded up, not a free parameter: within a factor 3 of what is measured (the integer term: exact)
    assert all(worst[name] >= 1.0 / 3.0 for name in R.TERMS[:3]), worst
    assert worst["contact_match"] == 0.0
    assert R.BUDGET_CLOCK / 3.0 <= worst_clock <= R.BUDGET_CLOCK


def test_every_foot_reaches_the_four_cells(sensed):
    """Scheduled stance or swing, times in contact or not: every foot has rows in each cell over the states and phases the GPU test of
    the fixture loads, with the command's stand gate off and on."""
    force, feet = sensed
    _, command, _, _ = R.extras(len(feet))
    cells = np.zeros((4, 2, 2), int)
    stood = matches = 0
    for view in _phases(R.SEEDS[0]):
        ref = R.evaluate(view, force, feet, **R.PARAMS)
        for f in range(4):
            for h in (0, 1):
                for c in (0, 1):
                    cells[f, h, c] += int(((ref["hard"][:, f] == h) & (ref["contact"][:, f] == c)).sum())
        gated = R.evaluate(view, force, feet, command=command, **R.PARAMS)
        stood += int((gated["hard"].all(1) & ~ref["hard"].all(1)).sum())
        matches |= 1 << int(ref["terms"][:, 3].max()) | 1 << int(ref["terms"][:, 3].min())
    print("rows per (foot, scheduled stance, contact):", cells.tolist(), "; envs the gate makes stand:", stood)
    assert (cells >= 20).all(), cells.tolist()
    assert stood >= 40 and matches & 1 and matches & 16                             # contact_match reaches 0 and 4
    # the 1- and 5-env prefixes hold both kinds of states
    contact = force[:, list(R.FEET), 2] > np.float32(R.FORCE_THRESHOLD)
    assert contact[:5].any() and not contact[:5].all()


def test_names_and_shared_parameters():
    assert R.TERMS == _abi.SCHED_TERMS and R.DIM == _abi.SCHED_DIM == 10 and R.SALT == int.from_bytes(b"QGSCHED1", "big")
    assert all(w != 0 for w in R.WEIGHTS.values()) and any(w > 0 for w in R.WEIGHTS.values()) and any(w < 0 for w in R.WEIGHTS.values())
    assert R.SIZES == (1, 5, 67) and R.STEPS == 40 and float(R.DT32) == float(np.float32(0.02)) and R.FREQ[1] * float(R.DT32) <= 0.5
    assert R.done_table(67).sum(0).max() == 4 and R.done_table(67)[:, ::5].sum() == 0
