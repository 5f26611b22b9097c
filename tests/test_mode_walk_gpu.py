"""A handle walked through its modes steps like a fresh one.

Every feature of the simulator handle is pinned numerically from a handle CREATED in the configuration under test.  Here a live handle
is taken from mode A into mode B with the API's own switches (tests/mode_walk.py: MODES, transition by features), a fresh twin is built
directly in B and given the walked handle's state through the public API only -- BatchedSim.snapshot / restore, WalkLayer.state /
load_state, ObsPack.state / load_state -- and both take the same env-steps through every step form of B.  Everything must be the same
BITS: every output of every step, the final snapshot (physics, reset streams, dynamics rows, wrench rows, layer blobs) and
last_step_kernel, which is also the name tests/kernel_leaves.py pins against the f64 oracle.  The task, the effective mapping and the
baked flag are not copied into the twin: the walked handle must have the ones a fresh handle has.  No tolerance is involved, except in
the oracle anchor (d), which uses TOL["A"] and close() of tests/parity.py.

(a) every ordered pair of modes at n = 37, one case per source mode (and the pairs of the table robot's modes);
(b) two rings through all modes at the two sizes where AUTO's mapping changes;
(c) seeded random walks over mode switches, masked resets, set_state(get_state()), snapshot / restore, set_track_ctrl and steps;
(d) for the modes the oracle can express, the first env-step after the transition against the oracle from the walked handle's
    read-back state (both handles wrong in the same way);
(e) every documented refusal: the call raises, the snapshot bytes are unchanged and the next env-steps are those of a twin that never
    saw the call.  A refusal met in (a) - (c) that EXPECTED_REFUSALS does not list fails the test.

With QG_MODE_WALK_OUT=<file> every transition appends a line: A -> B, n, kernel, forms compared, resets seen."""
import os

import numpy as np
import pytest

from quadruped_gym_amd import _abi

import mode_walk as W
import parity
from helpers import env_model, write_table_robot
from kernel_leaves import LEAVES, MULTI_TWINS
from mode_walk import EXPECTED_REFUSALS, expected_refusal
from parity import TOL, close

pytestmark = pytest.mark.gpu

RECORD = "QG_MODE_WALK_OUT"


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def simds():
    return parity.simds()


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from quadruped_gym_amd.model.loader import load_model
    return {"baked": None, "table": load_model(write_table_robot(tmp_path_factory.mktemp("robot")))[0]}


def record(line):
    path = os.environ.get(RECORD)
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


# ---- (d) the oracle anchor -------------------------------------------------------------------------------------------------------------
def oracle_anchor(oracle, sim, snap, acts0, out, what):
    """The first env-step after the transition against the f64 oracle started from the walked handle's read-back state."""
    s = snap["sim"]
    n, task, t = sim.n, sim.get_task(), TOL["A"]
    rows = s.get("dynamics")
    cols = ([], [], [], [], [], [])
    for lo, hi in ((0, n),) if rows is None else tuple((i, i + 1) for i in range(n)):
        b = oracle.Batch(sim.model if rows is None else env_model(oracle, sim.model, rows[lo]), task, hi - lo)
        b.set_state(*(s[k][lo:hi].astype(np.float64) for k in ("qpos", "qvel", "act", "ctrl")), s["nstep"][lo:hi])
        obs, rew, done, _ = b.step(acts0[lo:hi].astype(np.float64))
        for col, x in zip(cols, (obs, rew, done) + tuple(b.get_state()[:3])):
            col.append(x)
    obs_o, rew_o, done_o, q_o, v_o, a_o = (np.concatenate(c) for c in cols)
    obs, rew, done = out["0.obs"], out["0.reward"], out["0.done"].astype(bool)
    mask = np.ones(obs.shape[1], bool)
    mask[12:15] = False
    close(obs[:, mask], obs_o[:, mask], t["obs"], what + " obs")
    close(obs[:, 12:15], obs_o[:, 12:15], t["accel"], what + " accelerometer")
    close(rew, rew_o, t["reward"], what + " reward")
    # terminations: only the envs whose termination is not within rounding of a threshold (the time limit is an integer test)
    sure = np.ones(n, bool)
    if task.use_fall:
        sure &= np.abs(q_o[:, 2] - task.fall_height) > 1e-4
    if task.use_flip:
        sure &= np.abs(obs_o[:, 29]) > 1e-4
    assert np.array_equal(done[sure], done_o[sure]), what + " done"
    keep = ~done & ~done_o                    # finished envs were auto-reset on the device
    assert keep.sum() >= n // 4, what
    close(out["0.qpos"][keep], q_o[keep], t["qpos"], what + " qpos")
    close(out["0.qvel"][keep], v_o[keep], t["qvel"], what + " qvel")
    close(out["0.act"][keep], a_o[keep], t["act"], what + " act")
    return int(keep.sum())


# ---- the differential check ------------------------------------------------------------------------------------------------------------
def twin_check(walked, model, robot, simds, seed, what, steps=W.SEQ_K, forms=None, oracle=None):
    """A fresh twin in the walked handle's configuration, its state through the public API, the same env-steps through every form.
    Returns (kernel of the first form, forms compared, done [steps, n] of the first form)."""
    feats, n = tuple(walked.features), walked.sim.n
    forms = forms or W.forms_of(feats)
    snap = W.snapshot(walked)
    twin = W.build(n, feats, model)
    try:
        # what is NOT copied: a walked handle has the task, the mapping and the baked flag of a fresh one
        assert W.task_fields(walked.sim.get_task()) == W.task_fields(twin.sim.get_task()), what + ": task"
        assert walked.sim.mapping == twin.sim.mapping, what + ": effective mapping"
        lib = walked.sim._lib
        assert walked.sim.baked == twin.sim.baked == bool(lib.qg_uses_baked_model(walked.sim._h)) == bool(lib.qg_uses_baked_model(twin.sim._h)), \
            what + ": baked flag"
        W.adopt(twin, snap, walked.track_ctrl)
        assert not W.differing(snap, W.snapshot(twin)), what + ": the twin's snapshot after restore"
        acts = W.actions(seed, steps, n)
        first = None
        for i, form in enumerate(forms):
            if i:       # (the first form runs on the walked handle as the transition left it)
                W.restore(walked, snap)
                W.restore(twin, snap)
            out_w, done_w = W.run_form(walked, form, acts)
            out_t, _ = W.run_form(twin, form, acts)
            where = f"{what} [{form}]"
            assert not W.differing(out_w, out_t), f"{where}: outputs differ at {W.differing(out_w, out_t)[:6]}"
            want = W.expected_kernel(feats, n, simds, form, robot)
            assert walked.sim.last_step_kernel == twin.sim.last_step_kernel == want, \
                f"{where}: kernels {walked.sim.last_step_kernel} / {twin.sim.last_step_kernel}, expected {want}"
            assert want in LEAVES or want in MULTI_TWINS, where
            end_w, end_t = W.snapshot(walked), W.snapshot(twin)
            assert not W.differing(end_w, end_t), f"{where}: final snapshots differ at {W.differing(end_w, end_t)}"
            if i == 0:
                first = (walked.sim.last_step_kernel, done_w)
                if oracle is not None and form == "step":
                    oracle_anchor(oracle, walked.sim, snap, acts[0], out_w, where)
        return first[0], forms, first[1]
    finally:
        twin.close()


def go(ctx, a, b, size):
    """The walked handle from A to B.  Returns the key of EXPECTED_REFUSALS if B refused (the handle is then as far as it got)."""
    try:
        W.switch(ctx, W.MODES[b].features)
    except _abi.QuadGymError as err:
        key = expected_refusal(err, a, b, size)
        assert key is not None, f"{a} -> {b} at n = {ctx.sim.n}: a refusal EXPECTED_REFUSALS does not list: {err}"
        return key
    return None


def reset_all(ctx, seed):
    flags = _abi.RESET_RANDOM_YAW
    if ctx.po is not None:
        ctx.po.reset(seed, flags)
    elif ctx.walk is not None:
        ctx.walk.reset(seed, flags)
    else:
        ctx.sim.reset(seed=seed, flags=flags)


def one_transition(a, b, n, robot, models, simds, oracle, seed):
    ctx = W.build(n, W.MODES[a].features, models[robot])
    try:
        ctx.set_track_ctrl(seed % 2 == 0)     # every other transition without the data.ctrl write-back (where no layer needs it)
        reset_all(ctx, seed)
        W.stagger(ctx.sim, W.PLAN_A)
        _, done_a = W.run_form(ctx, W.MODES[a].forms[0], W.actions(seed, 3, n))
        assert go(ctx, a, b, "small") is None
        W.stagger(ctx.sim, W.PLAN_B)          # (binding a walking layer resets the robots: the stagger again, for the steps in B)
        what = f"{a} -> {b} n={n} {robot}"
        kernel, forms, done_b = twin_check(ctx, models[robot], robot, simds, seed + 1, what, oracle=oracle if W.MODES[b].oracle else None)
        assert kernel == W.MODES[b].kernel(n, simds, robot=robot)
        in_a, in_b = done_a.any(0), done_b.any(0)
        assert in_a.any() and in_b.any() and (~in_a & ~in_b).any(), f"{what}: resets in A {in_a.sum()}, in B {in_b.sum()}"
        record(f"{a} -> {b} n={n} {robot} {kernel} forms={','.join(forms)} resets A={int(in_a.sum())} B={int(in_b.sum())} "
               f"neither={int((~in_a & ~in_b).sum())} track_ctrl={int(ctx.track_ctrl)}")
    finally:
        ctx.close()


# ---- (a) every ordered pair ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", W.ORDER)
def test_walked_handle_steps_like_a_fresh_one(oracle, models, simds, a):
    for k, (src, b) in enumerate(W.TRANSITIONS):
        if src == a:
            one_transition(a, b, W.N_SMALL, "baked", models, simds, oracle, seed=20 + k)


@pytest.mark.parametrize("a", W.TABLE_MODES)
def test_walked_handle_steps_like_a_fresh_one_on_the_table_robot(oracle, models, simds, a):
    for k, (src, b) in enumerate(W.TABLE_TRANSITIONS):
        if src == a:
            one_transition(a, b, W.N_SMALL, "table", models, simds, oracle, seed=200 + k)


# ---- (b) the AUTO boundaries ----------------------------------------------------------------------------------------------------------
def short_forms(features):
    """(b) and (c): the first form (host buffers, the state read back after every step) and the last one (device buffers)."""
    forms = W.forms_of(features)
    return (forms[0], forms[-1])


@pytest.mark.parametrize("direction", sorted(W.RINGS))
@pytest.mark.parametrize("size", sorted(W.BOUNDARY_SIZES))
def test_rings_through_every_mode_at_the_auto_boundaries(oracle, models, simds, size, direction):
    n = W.BOUNDARY_SIZES[size](simds)
    ctx = W.build(n, (), None)
    try:
        reset_all(ctx, 31)
        for k, (a, b) in enumerate(W.RINGS[direction]):
            refused = go(ctx, a, b, size)
            W.stagger(ctx.sim, W.PLAN_B)
            what = f"ring {direction} {a} -> {b} n={n}"
            # (d) at the first boundary only: per-env dynamics cost one oracle model per env, and every leaf of the second boundary
            # is held to the oracle at that size by tests/test_kernel_leaves_gpu.py
            anchored = oracle if (W.MODES[b].oracle and not refused and n <= W.BOUNDARY_SIZES["first_quad"](simds)) else None
            kernel, forms, done_b = twin_check(ctx, None, "baked", simds, 300 + k, what, forms=short_forms(ctx.features), oracle=anchored)
            if not refused:
                assert kernel == W.MODES[b].kernel(n, simds)
            record(f"{what} {kernel} forms={','.join(forms)} resets B={int(done_b.any(0).sum())}" + (f" REFUSED: {refused}" if refused else ""))
            if refused:
                W.switch(ctx, ())       # the ring goes on from the plain handle
    finally:
        ctx.close()


# ---- (c) seeded random walks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", sorted(W.WALK_SIZES))
@pytest.mark.parametrize("seed", W.WALK_SEEDS)
def test_seeded_random_walks(models, simds, seed, size):
    n = W.WALK_SIZES[size](simds)
    ctx = W.build(n, (), None)
    current, trail = "M0", []
    try:
        reset_all(ctx, 41 + seed)
        W.stagger(ctx.sim, W.PLAN_B)
        for j, op in enumerate(W.random_walk(seed)):
            if op[0] == "mode":
                refused = go(ctx, current, op[1], size)
                current = op[1]
                if refused:
                    W.switch(ctx, ())
                    current = "M0"
                W.stagger(ctx.sim, W.PLAN_B)
                trail.append(op[1] + ("(refused)" if refused else ""))
            elif op[0] == "reset":
                mask = np.random.default_rng(op[1]).random(n) < 0.3
                flags = ctx.sim.get_task().reset_flags
                top = ctx.po if ctx.po is not None else ctx.walk
                if top is not None:
                    top.reset(0, flags, mask)
                else:
                    ctx.sim.reset(mask=mask, flags=flags)
                trail.append("reset")
            elif op[0] == "set_get":
                ctx.sim.set_state(*ctx.sim.get_state())
                trail.append("set_get")
            elif op[0] == "snap_restore":
                W.restore(ctx, W.snapshot(ctx))
                trail.append("snap_restore")
            elif op[0] == "track_ctrl":
                ctx.set_track_ctrl(not ctx.track_ctrl)
                trail.append(f"track_ctrl={int(ctx.track_ctrl)}")
            else:
                forms = W.forms_of(ctx.features)
                form = forms[op[1] % len(forms)]
                W.run_form(ctx, form, W.actions(op[2], 1, n))
                trail.append(form)
            if (j + 1) % W.WALK_CHECK_EVERY == 0:
                what = f"walk seed={seed} n={n} after op {j + 1} in {current} ({' '.join(trail[-W.WALK_CHECK_EVERY:])})"
                kernel, forms, done_b = twin_check(ctx, None, "baked", simds, 500 + 31 * seed + j, what, forms=short_forms(ctx.features))
                record(f"{what} {kernel} forms={','.join(forms)} resets B={int(done_b.any(0).sum())}")
    finally:
        ctx.close()


# ---- (e) a refused call leaves no trace --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(EXPECTED_REFUSALS))
def test_a_refused_call_leaves_no_trace(models, simds, key):
    r = EXPECTED_REFUSALS[key]
    n = W.N_SMALL if r.size == "small" else W.BOUNDARY_SIZES[r.size](simds)
    feats = W.MODES[r.mode].features
    ctx = W.build(n, feats, models[r.robot])
    twin = None
    try:
        reset_all(ctx, 51)
        W.stagger(ctx.sim, W.PLAN_B)
        lead = W.forms_of(feats)[0]
        W.run_form(ctx, lead, W.actions(60, 1, n))
        before = W.snapshot(ctx)
        with pytest.raises(_abi.QuadGymError) as info:
            r.call(ctx)
        assert r.quote in str(info.value), str(info.value)
        assert r.quote in open(os.path.join(W.CSRC, r.source)).read()
        del info
        assert tuple(ctx.features) == feats
        assert not W.differing(before, W.snapshot(ctx)), "the snapshot bytes after the refused call"
        twin = W.build(n, feats, models[r.robot])
        W.adopt(twin, before, ctx.track_ctrl)
        acts = W.actions(61, 2, n)
        out_w, _ = W.run_form(ctx, lead, acts)
        out_t, _ = W.run_form(twin, lead, acts)
        assert not W.differing(out_w, out_t), f"outputs differ at {W.differing(out_w, out_t)[:6]}"
        assert ctx.sim.last_step_kernel == twin.sim.last_step_kernel == W.expected_kernel(feats, n, simds, lead, r.robot)
        assert not W.differing(W.snapshot(ctx), W.snapshot(twin))
    finally:
        if twin is not None:
            twin.close()
        ctx.close()
