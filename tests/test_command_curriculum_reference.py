"""The command curriculum's definition (tests/command_curriculum_reference.py) without a GPU: the inverse CDF's shares over all 2^24
draws, the neighbour sets, a census of the scripted table -- conditions on the INPUTS the GPU test replays, met by the reference alone --
and the float32 budget of the command floats, measured here against float64 and compared with what the module records."""
import numpy as np

import command_curriculum_reference as R


def test_bin_shares_over_all_draws():
    """Over all 2^24 values of k(0) the bins' counts are the weights' shares to within one count, and a bin of weight 0 is never drawn:
    arithmetically for several weight vectors, and by running draw_bin over every value for two of them."""
    rng = np.random.default_rng(3)
    vectors = [np.array(R.MAIN["initial_weights"]), np.array([1]), np.array([3, 0, 0, 5, 65536, 1, 0, 2]), np.array(R.WIDE["initial_weights"]),
               np.full(256, 65536), rng.integers(0, 65537, 256), rng.integers(0, 13, 12)]
    for w in vectors:
        counts, T = R.bin_counts(w), int(w.sum())
        assert counts.sum() == 1 << 24 and (counts[w == 0] == 0).all()
        share = w.astype(np.float64) * 2.0 ** 24 / T
        assert (np.abs(counts - share) <= 1.0).all(), np.abs(counts - share).max()
    every = np.arange(1 << 24, dtype=np.int64)
    for w in (vectors[2], vectors[6]):
        got = np.bincount(R.draw_bin(every, w), minlength=len(w))
        assert np.array_equal(got, R.bin_counts(w))
    # the ends: k0 = 0 draws the first bin with a weight, k0 = 2^24 - 1 the last one
    w = np.array([0, 4, 0, 7, 0])
    assert R.draw_bin(np.array([0, (1 << 24) - 1]), w).tolist() == [1, 3]


def test_neighbour_sets():
    N = R.neighbours
    assert N(0, 1, 1) == [0]
    assert N(0, 1, 5) == [0, 1, 4] and N(4, 1, 5) == [0, 3, 4] and N(2, 1, 5) == [1, 2, 3]          # 1 x N: the angle wraps
    assert N(0, 1, 2) == [0, 1] == N(1, 1, 2)                                                       # two angle bins: a set, counted once
    assert N(0, 5, 1) == [0, 1] and N(4, 5, 1) == [3, 4] and N(2, 5, 1) == [1, 2, 3]                # N x 1: the speed does not
    assert N(0, 2, 2) == [0, 1, 2] and N(3, 2, 2) == [1, 2, 3]
    assert N(0, 16, 16) == [0, 1, 15, 16] and N(255, 16, 16) == [239, 240, 254, 255]
    assert N(17, 16, 16) == [1, 16, 17, 18, 33] and N(16 * 7 + 15, 16, 16) == [16 * 6 + 15, 16 * 7, 16 * 7 + 14, 16 * 7 + 15, 16 * 8 + 15]
    for ns, na in ((1, 1), (1, 7), (7, 1), (2, 2), (3, 4), (16, 16)):                                 # symmetric, and sized as counted
        for c in range(ns * na):
            assert all(c in N(b, ns, na) for b in N(c, ns, na))
            assert len(N(c, ns, na)) == 1 + (c // na > 0) + (c // na < ns - 1) + (na >= 2) + (na >= 3)


def test_grid_edges():
    s, a = R.edges(R.MAIN["speed"], R.MAIN["bins"])
    assert s.dtype == a.dtype == np.float32 and len(s) == 4 and len(a) == 5
    assert s[0] == np.float32(0.1) and a[0] == -R.PI32 and abs(float(s[-1]) - 1.0) < 2e-7 and abs(float(a[-1]) - np.pi) < 1e-6
    s, _ = R.edges(R.ONE["speed"], R.ONE["bins"])
    assert s[0] == s[1] == np.float32(0.3)                        # a degenerate range: every draw is speed_lo


def test_census_of_the_scripted_table():
    n = R.SIZES["main"]
    cur = R.Curriculum(n, **R.MAIN)
    ns, na = cur.shape
    done, comps = R.table(n)
    assert (cur.weight > 0).sum() == 1 and cur.weight[0] > 0 and (cur.bin == 0).all()          # one unlocked bin
    seen = dict(clamp=False, twice=False, idle=False, wrap=False, by_done=False, by_steps=False, short=False)
    nan_failed = {row: False for row in R.NAN_ROWS}
    start = np.zeros(n, np.int64)                                 # the env-step (1-based) each running segment began at
    for t in range(1, R.STEPS + 1):
        out = cur.advance(done[t - 1], comps[t - 1])
        ended, success = out["ended"], out["success"]
        seen["idle"] |= not ended.any()
        seen["twice"] |= bool((out["s_b"] >= 2).any())
        seen["clamp"] |= bool((cur.weight == cur.W).any())
        seen["by_done"] |= bool((ended & out["by_done"]).any())
        seen["by_steps"] |= bool((ended & ~out["by_done"]).any())
        # a success at angle index 0 raises index n_alpha - 1: a launch whose successes all lie at ai = 0 lifts a bin at ai = n_alpha - 1
        hit = np.flatnonzero(out["s_b"])
        if len(hit) and (hit % na == 0).all():
            last = (hit // na) * na + na - 1
            seen["wrap"] |= bool((cur.weight[last] > out["before"][last]).any())
        # a segment that meets every criterion but is shorter than min_steps fails
        for i in np.flatnonzero(ended & ~success):
            rows = comps[start[i]:t, i].astype(np.float64)
            length = t - start[i]
            meets = rows[:, 2].sum() >= 0.5 * length + 1e-3 and rows[:, 5].sum() <= 0.25 * length - 1e-3
            seen["short"] |= bool(meets and length < cur.min_steps)
            for row in R.NAN_ROWS:
                if row[1] == i and start[i] < row[0] <= t and length >= cur.min_steps:
                    clean = np.nan_to_num(rows, nan=1.0 if row[2] == 2 else 0.0)
                    nan_failed[row] |= bool(clean[:, 2].sum() >= 0.5 * length + 1e-3 and clean[:, 5].sum() <= 0.25 * length - 1e-3)
        start[ended] = t
    assert all(seen.values()), seen
    assert all(nan_failed.values()), nan_failed                   # each NaN row failed a segment that was long enough and otherwise good
    assert (cur.weight > 0).all() and (cur.weight == cur.W).any()  # every bin of the 3 x 4 grid unlocked by the end
    assert cur.episodes.sum() == cur.segment.sum() and (cur.successes <= cur.episodes).all() and cur.successes.sum() > 0
    assert len(np.unique(cur.bin)) == ns * na                     # and drawn from


def test_other_grids_run_the_table():
    """The 1 x 1 grid without criteria (min_steps alone decides) and the 16 x 16 grid: the state stays within its limits."""
    for name in ("one", "wide"):
        n = R.SIZES[name]
        params = getattr(R, name.upper())
        cur = R.Curriculum(n, **params)
        done, comps = R.table(n)
        for t in range(R.STEPS):
            cur.advance(done[t], comps[t])
        assert (cur.weight >= np.array(params["initial_weights"][:cur.B])).all() and (cur.weight <= cur.W).all()
        assert cur.episodes.sum() == cur.segment.sum() > 0 and (cur.bin < cur.B).all()
        if name == "one":
            assert cur.weight[0] == cur.W and (cur.speed == np.float32(0.3)).all() and cur.successes[0] == cur.episodes[0]
        else:
            assert (cur.weight > 0).sum() > 16 and (cur.speed >= 0).all() and (cur.speed <= np.float32(2.0) + 1e-6).all()
            assert (np.abs(cur.alpha) <= np.float32(np.pi) + 1e-6).all() and (np.abs(cur.theta) <= np.pi).all()


def test_begin_discards_unjudged():
    cur = R.Curriculum(20, **R.MAIN)
    done, comps = R.table(20)
    cur.advance(done[0], comps[0])
    before = (cur.weight.copy(), cur.episodes.copy(), cur.bin.copy(), cur.segment.copy())
    mask = np.arange(20) % 3 == 0
    cur.begin(mask)
    assert np.array_equal(cur.weight, before[0]) and np.array_equal(cur.episodes, before[1])
    assert np.array_equal(cur.segment, before[3] + mask) and (cur.steps[mask] == 0).all() and (cur.steps[~mask] == 1).all()
    assert not cur.sum[:, mask].any() and cur.sum[:, ~mask].any()


def test_float32_budget_of_the_command_floats():
    """The measurement the module records: float32 command floats against float64 on the same float32 (speed, alpha, theta)."""
    n = 1 << 16
    cur = R.Curriculum(n, **dict(R.WIDE, initial_weights=(1,) * 256))
    c64, c32 = cur.commands(), R.commands32(cur.speed, cur.alpha, cur.theta).astype(np.float64)
    scale = np.maximum(np.abs(cur.speed.astype(np.float64)), 2.0 ** -126)
    err = np.abs(c32 - c64)
    measured = {"velocity": float((err[:, 0:2] / scale[:, None]).max()), "heading": float(err[:, 2:4].max()),
                "global_velocity": float((err[:, 4:6] / scale[:, None]).max())}
    for name, value in measured.items():
        print("%s: measured %.3e, recorded budget %.3e (share %.2f)" % (name, value, R.BUDGET_COMMAND[name], value / R.BUDGET_COMMAND[name]))
        assert value <= R.BUDGET_COMMAND[name], name
        assert value >= 0.25 * R.BUDGET_COMMAND[name], name       # the record is a measurement, not a guess far above it
    assert (err <= R.command_tolerance(cur.speed)).all()
    assert len(np.unique(cur.bin)) == 256
