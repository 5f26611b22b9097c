"""The contact-cell fixture (tests/golden/contact_cells.npz, built by tests/contact_cells.py) reaches what it is there to reach.  No GPU.

Every condition is read from the f32 states by the census (``oracle.kinematics`` and the oracle's ``Diag`` over the four substeps of
one env-step): all 108 sample points touch the floor, grazing and pressed; the point a state is built for is the deepest of its body,
and alone on it for most points; nothing is pressed in beyond the caps; the cull-edge states stand on the farthest point; every body
takes every branch of the contact law; and moving any cp[b][i] by 1 mm moves the ORACLE's step by more than twice TOL["A"] in at least
one state of every cell of that point -- so a kernel with a wrong constant there cannot pass tests/test_parity_gpu.py::
test_every_contact_point_matches_oracle."""
import os

import numpy as np
import pytest

import contact_cells as CC
from parity import TOL


@pytest.fixture(scope="module")
def fix():
    return CC.load()


@pytest.fixture(scope="module")
def cen(oracle, fix):
    return CC.census(oracle, oracle.default_model(), fix, labels=fix)


def test_fixture_is_what_the_generator_produces(oracle, fix):
    again = CC.generate(oracle, TOL["A"])
    assert sorted(again) == sorted(fix) == sorted(CC.STATE_KEYS + CC.LABEL_KEYS)
    for k in again:
        assert again[k].dtype == fix[k].dtype and np.array_equal(again[k], fix[k]), k
    assert fix["qpos"].dtype == np.float32 and os.path.getsize(CC.FIXTURE) < 1 << 20


def test_every_cell_is_covered(oracle, fix, cen):
    model = oracle.default_model()
    cells = CC.cell_index(fix)
    assert len(cells) == 216 == 2 * int(cen["valid"].sum())
    alone_points = set()
    for (b, i, d), idx in sorted(cells.items()):
        assert 2 <= len(idx) <= 3, CC.cell_name(b, i, d)
        lo, hi = CC.DEPTH_RANGE[d]
        for e in idx:
            pen = cen["start_depth"][e, b, :model.ncp[b]]
            assert lo <= pen[i] <= hi, (CC.cell_name(b, i, d), pen[i])
            assert pen[i] - np.delete(pen, i).max() >= 0.9 * CC.MIN_GAP, CC.cell_name(b, i, d) + ": the point is the deepest of its body"
            assert cen["touch"][e, b, i]
            if cen["alone"][e, b, i]:
                alone_points.add((b, i))
    print(f"points with a state in which they are alone on their body: {len(alone_points)} of 108")
    assert len(alone_points) >= CC.MIN_ALONE_POINTS
    assert cen["untouched"] == 0 and (cen["hits"][cen["valid"]] >= 4).all()


def test_depth_caps(cen):
    deep = cen["deep_cells"]
    print(f"deepest state {1e3 * cen['deepest'].max():.1f} mm; {len(deep)} of 216 cells above {1e3 * CC.SOFT_DEPTH:.0f} mm:")
    for b, i, d, depth in deep:
        print(f"    {CC.cell_name(b, i, d)}: {1e3 * depth:.1f} mm")
    assert cen["deepest"].max() <= CC.HARD_DEPTH
    assert len(deep) <= CC.MAX_DEEP_CELLS


def test_cull_edge_states(oracle, fix, cen):
    """One state per link in which its farthest sample point points straight down and grazes the floor.  The FRAME has none: the best
    pose the search finds with a corner straight down presses a leg in beyond the hard cap."""
    model = oracle.default_model()
    edge = {(int(fix["body"][e]), int(fix["point"][e])): int(e) for e in np.flatnonzero(fix["kind"] == CC.KIND_EDGE)}
    want = [(b, i) for b, i in CC.edge_cells(model) if b > 0]
    assert sorted(edge) == sorted(want) and {b for b, _ in want} == set(range(1, 13))
    cps = CC.sample_points(model)
    for (b, i), e in edge.items():
        assert np.linalg.norm(cps[b][i]) == np.linalg.norm(cps[b], axis=1).max()
        assert CC.edge_tilt(oracle, model, fix["qpos"][e], b, i) < 1e-5                  # f32 quaternion: ~1e-7 rad
        pen = cen["start_depth"][e, b, :model.ncp[b]]
        assert CC.EDGE_RANGE[0] <= pen[i] <= CC.EDGE_RANGE[1] and np.delete(pen, i).max() < 0, (b, i, pen)
        assert cen["deepest"][e] <= CC.SOFT_DEPTH
    # the FRAME: with a corner straight down the hinge search (the generator's) finds no pose within 1.5 x the hard cap
    placer = CC.Placer(oracle, model)
    for b, i in CC.edge_cells(model):
        if b == 0:
            down = -cps[0][i] / np.linalg.norm(cps[0][i])
            _, _, deepest = placer.search(0, i, down[None], 5e-5, np.random.default_rng(i), free_u=False)
            assert deepest > 1.5 * CC.HARD_DEPTH


def test_every_body_takes_every_branch(cen):
    count = cen["branch"].sum(0)
    print("states per body (rows) and branch (%s):\n%s" % (", ".join(CC.BRANCHES), count))
    assert (count >= CC.MIN_BRANCH_STATES).all()


def test_each_cell_catches_a_wrong_constant(oracle, fix):
    """cp[b][i] moved by 1 mm along +-x, +-y, +-z: for every cell (point and depth class) and every shift, some state of the cell moves
    the oracle's env-step by more than MARGIN = 2 x TOL["A"] in qpos, qvel, obs or the accelerometer.  A point may fall back on 2 mm
    (over the states of its two cells); at most 11 may, and each is named with what it reached."""
    per_cell, one, two = CC.shift_coverage(oracle, fix, TOL["A"])
    assert len(per_cell) == 216 and len(one) == 108
    for d in (CC.GRAZE, CC.PRESS):
        weakest = min((k for k in per_cell if k[2] == d), key=lambda k: per_cell[k].min())
        print(f"1 mm shifts, weakest {CC.DEPTH_NAMES[d]} cell: {CC.cell_name(*weakest)}: {np.round(per_cell[weakest], 2)} x TOL "
              f"({', '.join(CC.SHIFT_NAMES)})")
    print(f"{len(two)} points on the 2 mm shift")
    for (b, i), ex in two.items():
        print(f"    body {b} point {i}: 1 mm {np.round(one[(b, i)], 2)}, 2 mm {np.round(ex, 2)} x TOL")
        assert (np.maximum(ex, one[(b, i)]) > CC.MARGIN).all(), (b, i)
    assert len(two) <= CC.MAX_WIDE_SHIFT_POINTS
    for (b, i, d), ex in per_cell.items():
        assert (b, i) in two or (ex > CC.MARGIN).all(), (CC.cell_name(b, i, d), ex)


def test_the_gap_this_fixture_closes(oracle, fix, cen):
    """The rollout and tilted-robot states of step_vectors.npz leave at least 30 of the 108 points in the air; with this fixture none."""
    gold = dict(np.load(CC.STEP_VECTORS))
    before = CC.census(oracle, oracle.default_model(), gold)
    print(f"points never on the floor: step_vectors.npz {before['untouched']} of 108, with contact_cells.npz "
          f"{int((cen['valid'] & (before['hits'] + cen['hits'] == 0)).sum())}")
    assert before["untouched"] >= 30
    assert not (cen["valid"] & (before["hits"] + cen["hits"] == 0)).any()
