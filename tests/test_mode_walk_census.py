"""The tables of the mode-walk test (tests/mode_walk.py, tests/test_mode_walk_gpu.py), checked without a GPU: every mode, every ordered
pair, every step form the header offers, every documented refusal, names that the leaf tables know, walks that enter every mode, and
step counters that give the resets the GPU test asks for -- on the f64 oracle alone."""
import os

import numpy as np

import mode_walk as W
from kernel_leaves import LEAVES, MULTI_TWINS

SIMDS = 1024                  # an MI355X
MODE_NAMES = ("M0", "M1", "M2", "M3", "M4", "M5", "M6", "M7", "M8", "M9", "M10")
# what the documented refusals cover: one entry of EXPECTED_REFUSALS at least per line
DOCUMENTED = ("set_mapping(LANE) with per-env dynamics", "set_mapping(PAIR) with external wrenches", "set_mapping(PAIR) on the table robot",
              "per-env dynamics on LANE", "external wrenches on PAIR", "set_task with a walking layer bound", "set_task with another obs_mode",
              "step_device_seq with a walking layer bound", "step_device_seq with per-env dynamics",
              "step_device_seq with external wrenches",
              "resident_start with an observation pack bound", "resident_start with external wrenches",
              "resident_start above one wave per SIMD", "set_mapping with the resident mode on", "a second walking layer",
              "reset(RESET_DYNAMICS) without a range")


def test_every_mode_and_every_ordered_pair_is_walked():
    assert tuple(W.MODES) == MODE_NAMES
    want = {(a, b) for a in MODE_NAMES for b in MODE_NAMES if a != b}
    assert len(want) == 110 and set(W.TRANSITIONS) == want and len(W.TRANSITIONS) == 110
    table = ("M0", "M1", "M4", "M7", "M8")
    assert W.TABLE_MODES == table
    assert set(W.TABLE_TRANSITIONS) == {(a, b) for a in table for b in table if a != b}
    for ring in W.RINGS.values():          # each ring visits every mode once and comes back
        assert len(ring) == 11 and {a for a, _ in ring} == set(MODE_NAMES) == {b for _, b in ring}
        assert all(ring[k][1] == ring[k + 1][0] for k in range(10)) and ring[0][0] == ring[-1][1] == "M0"
    assert W.RINGS["reversed"] == tuple((b, a) for a, b in reversed(W.RINGS["forward"]))
    assert W.N_SMALL % 4 and W.N_SMALL % 16 and W.N_SMALL % 32        # a ragged last wave in every mapping
    assert [f(SIMDS) for f in W.BOUNDARY_SIZES.values()] == [4097, 16385]


def test_every_expected_kernel_is_a_known_instantiation():
    known = set(LEAVES) | set(MULTI_TWINS)
    sizes = [W.N_SMALL] + [f(SIMDS) for f in W.BOUNDARY_SIZES.values()]
    seen = set()
    for mode in W.MODES.values():
        for robot in ("baked", "table") if mode.table else ("baked",):
            for n in sizes if robot == "baked" else sizes[:1]:
                if "resident" in mode.features and n > W.N_SMALL:
                    continue                  # refused there (EXPECTED_REFUSALS)
                assert mode.kernel(n, SIMDS, robot=robot) in known, (mode.name, n, robot)
                for form in mode.forms:
                    name = mode.kernel(n, SIMDS, form, robot)
                    assert name in known, (mode.name, n, form, robot, name)
                    seen.add(name)
    assert len(seen) >= 25          # the walk goes through the leaves, not round them


def test_every_step_form_of_the_header_is_walked():
    assert W.header_step_entries() == set(W.FORMS.values())
    blocked_seq = [set(W.MODES[r.mode].features) for r in W.EXPECTED_REFUSALS.values() if r.call is W._seq]
    needs = {"resident": "resident", "walk_step": "walk", "walk_step_device": "walk", "po_step": "po", "po_step_device": "po"}
    for mode in W.MODES.values():
        assert len(set(mode.forms)) == len(mode.forms)
        for form in set(W.FORMS) - set(mode.forms):
            if form == "step_device_seq":       # left out only where a listed refusal says so
                assert any(set(mode.features) & f for f in blocked_seq), (mode.name, form)
            else:
                assert needs[form] not in mode.features, (mode.name, form)
        assert mode.forms[0] in ("step", "walk_step", "po_step")       # the form that reads the state back after every env-step


def test_expected_refusals_are_documented_and_reached():
    assert set(W.EXPECTED_REFUSALS) == set(DOCUMENTED)
    ring_pairs = {p for ring in W.RINGS.values() for p in ring}
    for key, r in W.EXPECTED_REFUSALS.items():
        assert r.mode in W.MODES and r.robot in ("baked", "table"), key
        assert r.size == "small" or r.size in W.BOUNDARY_SIZES, key
        assert r.robot == "baked" or W.MODES[r.mode].table, key
        assert r.quote in open(os.path.join(W.CSRC, r.source)).read(), key
        reached = 0
        for a, b, size in r.during:
            assert a in W.MODES and b in W.MODES and a != b, key
            in_ring = size in W.BOUNDARY_SIZES and (a, b) in ring_pairs
            in_walk = size in W.WALK_SIZES and size != "small"
            assert in_ring or in_walk, (key, a, b, size)
            reached += in_ring
        assert not r.during or reached, key
    # the header says what the library refuses; the sentences quoted from the sources stand behind these
    header = open(W.HEADER).read()
    for words in ("refused without a range", "qg_set_mapping refuses it for other model numbers", "a second qg_walk_create on the same sim is refused",
                  "qg_step_device_seq and the resident form are refused, as are the PAIR and LANE",
                  "exists for the one-link-per-lane mapping (<= 4096 envs) only"):
        assert words in header, words


def test_walks_are_pure_functions_of_the_seed_and_enter_every_mode_twice():
    entered = {m: 0 for m in W.MODES}
    for seed in W.WALK_SEEDS:
        ops = W.random_walk(seed)
        assert ops == W.random_walk(seed) and len(ops) == W.WALK_OPS == 30
        assert {op[0] for op in ops} <= {"mode", "reset", "set_get", "snap_restore", "track_ctrl", "step"}
        for op in ops:
            if op[0] == "mode":
                entered[op[1]] += 1
    assert min(entered.values()) >= 2, entered
    kinds = {op[0] for seed in W.WALK_SEEDS for op in W.random_walk(seed)}
    assert kinds == {"mode", "reset", "set_get", "snap_restore", "track_ctrl", "step"}
    assert W.WALK_SEEDS == (0, 1, 2, 3) and set(W.WALK_SIZES) == {"small", "first_quad"}


def test_the_step_counters_give_the_resets_on_the_oracle_alone(oracle):
    """3 env-steps in A and 4 in B with the staggered step counters of mode_walk.stagger, on the f64 oracle with M0's task: some envs
    finish inside A, some inside B, some in neither (the oracle does not auto-reset: finished envs are reset by hand)."""
    n = W.N_SMALL
    task = oracle.default_task()
    task.frame_skip, task.max_time, task.use_time_limit = W.FRAME_SKIP, W.MAX_TIME, 1
    model = oracle.default_model()
    limit = oracle.time_limit_substeps(model.timestep, task.max_time)
    assert limit == 100 and limit > W.FRAME_SKIP * (max(W.PLAN_A) + 7)        # an env reset on the way does not finish a second time
    b = oracle.Batch(model, task, n)
    b.reset()

    def stagger(plan):
        q, v, a, c, _ = b.get_state()
        k = np.asarray(plan)[np.arange(n) % 4]
        b.set_state(q, v, a, c, np.where(k > 0, limit - W.FRAME_SKIP * k, 0))

    def run(steps, seed):
        seen = np.zeros(n, bool)
        for act in W.actions(seed, steps, n):
            assert np.abs(act).max() <= 1.3
            done = b.step(act.astype(np.float64))[2]
            b.reset(mask=done)
            seen |= done
        return seen
    stagger(W.PLAN_A)
    in_a = run(3, 1)
    stagger(W.PLAN_B)
    in_b = run(4, 2)
    assert in_a.any() and in_b.any() and (~in_a & ~in_b).any()
    assert np.array_equal(in_a, np.arange(n) % 4 == 0) and np.array_equal(in_b, np.arange(n) % 4 < 2)
