"""The state pools of the leaf tests (tests/test_kernel_leaves_gpu.py: module docstring), how they are laid out over a grid, and what a
walking / PO leaf is compared with.  Nothing in here needs a GPU: tests/test_po_step_reference.py runs the checker's own tests on
exactly these states, and tests/test_external_wrench_gpu.py steps the first pool through the per-env-dynamics leaves."""
import os
import sys

import numpy as np
import pytest

from quadruped_gym_amd import _abi

import contact_cells as CC
import po_step_reference as R
from helpers import env_model
from kernel_leaves import PO_WINDOW
from parity import GOLD, TOL

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from make_golden import sample_states  # noqa: E402  (seeded random-action rollout states; the other tests that draw some take it from here)

M_SAMPLE, M_CONTACT, BLOCK, TAIL = 256, 32, 64, 16
RECORD = "QG_PO_PARITY_OUT"

UPRIGHT = 0.05                 # z component of the base's z axis above which a built state counts as upright (3 degrees from lying on its side)
# the points of the second pool that only touch the floor with the robot on its back: the FRAME's top corners and top face, and
# points 0, 2, 5 and 7 of every femur.  Every state of their cells ends a walking / PO episode (flip termination), so those leaves
# step them at the front only; the plain-step leaves put them into blocks
ONLY_ON_ITS_BACK = {(0, i) for i in (0, 1, 2, 3, 8, 9, 10, 11)} | {(b, i) for b in (1, 4, 7, 10) for i in (0, 2, 5, 7)}


def _upright(qpos):
    return 1.0 - 2.0 * (qpos[..., 4] ** 2 + qpos[..., 5] ** 2) > UPRIGHT


def cell_contact_states(oracle):
    """The contact part of the second pool, from tests/golden/contact_cells.npz: the cull-edge states, then one state per sample point
    of the FRAME and of the femurs -- of the point's cells the first pressed state that stands upright (the walking and PO leaves end
    the episode of a robot on its back), else the first grazing one that does, else the first pressed one.  Returns the states, their
    (kind, body, point) labels and which of them stand upright."""
    fix = CC.load()
    cells = CC.cell_index(fix)
    pick = [int(e) for e in np.flatnonzero(fix["kind"] == CC.KIND_EDGE)]
    assert len(pick) == 16
    for b in (0, 1, 4, 7, 10):
        for i in range(12 if b == 0 else 8):
            cand = cells[(b, i, CC.PRESS)] + cells[(b, i, CC.GRAZE)]
            up = [e for e in cand if _upright(fix["qpos"][e])]
            pick.append(up[0] if up else cand[0])
    pick = np.array(pick)
    label = np.stack([fix[k][pick] for k in ("kind", "body", "point")], 1)
    up = _upright(fix["qpos"][pick])
    cellpts = label[:, 0] == CC.KIND_CELL
    assert {(int(b), int(i)) for _, b, i in label[cellpts & ~up]} == ONLY_ON_ITS_BACK
    return [fix[k][pick] for k in ("qpos", "qvel", "act", "nstep")], label, up


def build_states(oracle, pool="golden"):
    """The leaf test's states, actions, per-env dynamics rows and -- for the walking and PO leaves -- the second step's actions and the
    commands (no GPU: tests/test_po_step_reference.py runs the checker's own tests on exactly these).  `pool`: "golden" or "cells"
    (tests/test_kernel_leaves_gpu.py: module docstring)."""
    model, task = oracle.default_model(), oracle.default_task()
    if pool == "golden":
        # the FRAME and femur contacts: the 2 x 32 contact_states of the golden fixture (drawing them takes minutes of rejection sampling)
        gold = np.load(GOLD)
        contact = [gold[k][-2 * M_CONTACT:] for k in ("qpos", "qvel", "act", "nstep")]
    else:
        contact, label, upright = cell_contact_states(oracle)
    q, v, a, ns = (np.concatenate(x) for x in zip(sample_states(model, task, M_SAMPLE, seed=61), contact))
    m = len(q)
    actions = np.random.default_rng(64).uniform(-1, 1, (m, 12)).astype(np.float32)
    census = oracle.contact_census(model, task.frame_skip, q, v, a, ns, actions, extra=0)
    frame, femur = census[:, :, 0].any(1), census[:, :, [1, 4, 7, 10]].any((1, 2))
    touch = frame | femur
    if pool == "golden":
        assert frame[M_SAMPLE:M_SAMPLE + M_CONTACT].sum() >= 24 and femur[M_SAMPLE + M_CONTACT:].sum() >= 24
        extra = {}
    else:
        cellpts = label[:, 0] == CC.KIND_CELL
        assert frame[M_SAMPLE:][cellpts & (label[:, 1] == 0)].all() and femur[M_SAMPLE:][cellpts & (label[:, 1] > 0)].all()
        touch[M_SAMPLE:] = True                               # the shins' and feet's cull-edge states take a block of their own too
        # the rollout states that touch with the FRAME or a femur leave this pool: the blocks go to the built states only (which of
        # them, per leaf, is up to the terminations: check_leaf asserts and prints it)
        stay = np.r_[~touch[:M_SAMPLE], np.ones(m - M_SAMPLE, bool)]
        q, v, a, ns, actions, touch = q[stay], v[stay], a[stay], ns[stay], actions[stay], touch[stay]
        m = len(q)
        extra = dict(built=np.flatnonzero(touch), label=label, upright=upright)
        assert len(extra["built"]) == len(label) == 60
    rows = np.tile(_abi.identity_dynamics_row(_abi.default_model()), (m, 1))
    rng = np.random.default_rng(65)
    rows[:, 0] = rng.uniform(0.3, 1.5, m)
    rows[:, 1] = rng.uniform(-0.05, 0.2, m)
    rows[:, 2:5] = rng.uniform(-0.01, 0.01, (m, 3))
    rows[:, 5:] = rng.uniform(0.7, 1.3, (m, 6))
    # walking / PO leaves: a second env-step from the same states with actions that reach beyond the clip, and a command per state
    rng = np.random.default_rng(66)
    actions2 = rng.uniform(-1.3, 1.3, (m, 12)).astype(np.float32)
    speed, alpha, theta = rng.uniform(0.2, 1.0, m), rng.uniform(-np.pi, np.pi, m), rng.uniform(-np.pi, np.pi, m)
    velocity = np.stack([speed * np.cos(alpha), speed * np.sin(alpha)], 1).astype(np.float32)
    heading = np.stack([np.cos(theta), np.sin(theta)], 1).astype(np.float32)
    return dict(state=(q, v, a, ns), actions=actions, touch=touch, rows=rows.astype(np.float32), m=m, actions2=actions2,
                velocity=velocity, heading=heading, pool=pool, **extra)


def walking_task(frame_skip=4, max_time=10.0):
    """The task a walking / PO env of the leaf test runs (envs/walking.py: flip and time-limit terminations, no fall)."""
    task = _abi.default_task()
    task.frame_skip, task.max_time, task.use_time_limit, task.use_fall, task.use_flip = frame_skip, max_time, 1, 0, 1
    return task


def _task_numbers(task):
    return (task.frame_skip, task.max_time, task.use_time_limit, task.use_fall, task.use_flip, task.sensor_lag, task.obs_mode)


def expected_chain(oracle, st, model, task, dyn):
    """The two env-steps of a walking / PO leaf on the checker: the reset stack, the outputs of both steps and the reward components'
    sensitivity per step.  One chain serves the walking and the PO leaves of one robot (the frames do not feed the reward)."""
    chk = R.StepChecker(oracle, st["m"], task.frame_skip, settling_time=0.0, obs_window=PO_WINDOW, unit_zero=True)
    reset_stack = chk.reset()                                   # commands are still zero when the env is reset
    chk.set_commands(st["velocity"], st["heading"])
    models = [env_model(oracle, model, row) for row in st["rows"]] if dyn else model
    schedule = [(st["state"], st["actions"]), (st["state"], st["actions2"])]
    sensitivity, outs = R.reward_sensitivity(chk, models, task, schedule, TOL["A"], patterns=8, seed=67)
    return dict(reset=reset_stack, outs=outs, sensitivity=sensitivity, dt=chk.dt)


def _chain_cache(oracle, states):
    """(robot, dyn) -> expected_chain, computed once per robot and shared by its leaves; prints the measured sensitivities."""
    cache = {}

    def get(robot, dyn, model, task):
        key = (robot, dyn)
        if key not in cache:
            c = expected_chain(oracle, states, model, task, dyn)
            c["task"] = _task_numbers(task)
            for k, row in enumerate(c["sensitivity"]):
                R.record(RECORD, f"sensitivity pool={states['pool']} robot={robot} dyn={int(dyn)} step={k + 1}: " + " ".join(f"{x:.3e}" for x in row))
            cache[key] = c
        c = cache[key]
        assert c["task"] == _task_numbers(task) == _task_numbers(walking_task()), "the walking and PO leaves run one task"
        return c
    return get


@pytest.fixture(scope="module")
def states(oracle):
    return build_states(oracle)


@pytest.fixture(scope="module")
def cell_states(oracle):
    return build_states(oracle, pool="cells")


@pytest.fixture(scope="module")
def chains(oracle, states):
    return _chain_cache(oracle, states)


@pytest.fixture(scope="module")
def cell_chains(oracle, cell_states):
    return _chain_cache(oracle, cell_states)


def layout(n, m, touch, tail_ok, block_ok=None):
    """State index of every env.  `tail_ok`: the states that may fill the blocks and the tail (they neither touch nor terminate);
    `block_ok`: the touching states that may be a block's one contact env (default: those of `tail_ok`)."""
    quiet = np.flatnonzero(~touch & tail_ok)
    contact = np.flatnonzero(touch & (tail_ok if block_ok is None else block_ok))
    idx = np.empty(n, np.int64)
    front = min(n, m)
    idx[:front] = np.arange(front)
    rest = np.arange(front, n)
    idx[rest] = quiet[rest % len(quiet)]
    blk, off = (rest - m) // BLOCK, (rest - m) % BLOCK
    one = off == (blk * 41 + 7) % BLOCK                   # 41: odd, so the position walks through all 64 lanes of the block
    idx[rest[one]] = contact[blk[one] % len(contact)]
    if n > 4 * TAIL:
        idx[-TAIL:] = quiet[np.arange(TAIL) % len(quiet)]
    return idx


def same_bits_wherever_it_sits(idx, touch, m, restarted, arrays):
    """A touching state's env in a block gives the bits of its env at the front (another lane, other neighbours in its wave): the
    wave-uniform contact skips and the femur cull change nothing for the env that does touch.  A grazing contact dropped by a skip
    moves the step by less than TOL["A"]; only this comparison sees it.  `restarted`: the envs a task layer restarted in the step
    with draws of their own (left out; a plain step restarts none).  `arrays`: name -> per-env array.  Returns how many envs were
    compared."""
    restarted = np.asarray(restarted, bool)
    later = np.flatnonzero(touch[idx] & (np.arange(len(idx)) >= m) & ~restarted)
    assert not restarted[idx[later]].any()
    for name, x in arrays.items():
        x = np.ascontiguousarray(x)
        here, front = (x[e].reshape(len(later), -1).view(np.uint8) for e in (later, idx[later]))
        bad = later[(here != front).any(1)]
        assert not len(bad), f"{name}: envs {bad[:8].tolist()} differ from the envs {idx[bad[:8]].tolist()} that hold the same touching states"
    return len(later)
