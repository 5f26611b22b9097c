"""Every per-launch step-kernel leaf (tests/kernel_leaves.py: LEAVES) against the f64 oracle, ONE env-step over the whole batch.

m seeded states -- random-action rollout states, 32 with the FRAME pressing on the floor and 32 with a femur doing so
(tools/make_golden.py: sample_states, and the contact_states of tests/golden/step_vectors.npz) -- are laid out over all n envs; identical states give identical bits in any lane, so every env is compared
with its state's oracle row at O(m) oracle cost.  The layout puts every state once at the front, then 64-env blocks of states
whose FRAME and femurs stay off the floor, each with exactly ONE FRAME- or femur-contact env at a lane position that moves from
block to block (the wave-uniform contact skips and the femur cull in both directions), and at the back states that neither touch
nor terminate (the last, partial workgroup holds one at n = 4097 and 32 769).  Tolerances: TOL["A"] of tests/parity.py.  The pools, the
layout and the expected chains live in tests/leaf_states.py, the handle builder in tests/kernel_leaves.py.

What is pinned per leaf.  Every leaf: qpos, qvel, act and the step counter.  Plain and walking leaves: the 33-value observation.  Plain
leaves: reward and terminations.  Walking AND partially observable leaves (tests/po_step_reference.py, a chain of the oracles that
takes nothing from the GPU: settling gate and clip -> C physics oracle -> walking reward on the ORACLE's sensors -> Madgwick frame and
FIFO on the oracle's sensors and quaternion): the 11 reward components and the reward, and for the PO leaves the WHOLE returned stack
of obs_window = 3 frames -- gyro, accelerometer, Euler angles, body velocity, data.ctrl, command, the frame's place in the FIFO and the
reset frames behind it.  Those leaves take a SECOND env-step from the same states with other actions (beyond the clip) and per-state
commands: the first step after a reset has a zero derived reward term (component 10) and a filter estimate that aliases qpos, the
second exercises both.  With QG_PO_PARITY_OUT=<file> every leaf appends its maxima per column group and reward component to that
file (profiles/r20/po_frame_parity.txt).

A SECOND POOL (``cell_states``; tests/contact_cells.py) runs through every leaf in the same layout with the same assertions: in place
of the 2 x 32 tilted-robot states it holds 60 built states -- the 16 cull-edge states (the farthest sample point of a femur, shin or
foot straight down, grazing the floor: what a bounding-sphere cull with too small a radius drops) and one state for every sample
point of the FRAME and of the four femurs (pressed, and upright where the point allows it) -- the per-point constants behind the
wave-uniform skips.  For both pools a FRAME- or femur-contact env gives the same bits wherever it sits: its rows in the blocks equal
its row at the front.

Which touching states become a block's contact env depends on the leaf.  A plain step does not restart an env that finishes and
compares it, so there every touching state may (a robot with its FRAME on the floor is below the fall height and finishes): all 60
built states, as many as the grid has blocks (59 at the one-link-per-lane sizes, 11 at n = 1000, all 60 once the grid has 60 blocks: the leaves of 16 383 envs and more).  The
walking and PO layers restart a finished env, so their blocks hold only states that end no episode in either step: of the built
states the 30 that stand upright (FRAME points 4-7, femur points 1, 3, 4 and 6, ten cull-edge states) and whatever else survives
(measured: one more cull-edge state, 31 in every such leaf of 4093 envs and more).
ONLY_ON_ITS_BACK names the points those leaves never see in a block -- the FRAME's top corners and top face and femur points 0, 2, 5
and 7 touch the floor only with the robot overturned, which the flip termination ends.  check_leaf asserts which built states land in
a block and prints the count."""
import numpy as np
import pytest

import contact_cells as CC
import po_step_reference as R
from helpers import oracle_per_env, table_robot  # noqa: F401  (table_robot: a fixture)
from kernel_leaves import LEAVES, PO_WINDOW, open_leaf
from leaf_states import RECORD, TAIL, cell_chains, cell_states, chains, layout, same_bits_wherever_it_sits, states  # noqa: F401  (fixtures)
from parity import TOL, close, simds

pytestmark = pytest.mark.gpu

CASES = [(name, k) for name, leaf in LEAVES.items() for k in range(len(leaf.sizes))]


def _handle(leaf, n, robot):
    """The handle (and the VecEnv, for walking / PO leaves) the row describes."""
    sim, env = open_leaf(leaf, n, robot, obs_window=PO_WINDOW)
    assert sim.baked == (leaf.robot == "baked")
    return sim, env


@pytest.mark.parametrize("name,k", CASES, ids=[f"{name}-{k}" for name, k in CASES])
def test_leaf_matches_oracle(oracle, states, chains, table_robot, name, k):
    check_leaf(oracle, states, chains, table_robot, name, k)


@pytest.mark.parametrize("name,k", CASES, ids=[f"{name}-{k}" for name, k in CASES])
def test_leaf_matches_oracle_on_contact_cells(oracle, cell_states, cell_chains, table_robot, name, k):
    """The second pool: cull-edge states and every sample point of the FRAME and the femurs (module docstring: which of them a leaf
    puts into blocks)."""
    check_leaf(oracle, cell_states, cell_chains, table_robot, name, k)


def check_leaf(oracle, states, chains, table_robot, name, k):
    leaf = LEAVES[name]
    n = leaf.sizes[k](simds())
    sim, env = _handle(leaf, n, table_robot)
    m, (q, v, a, ns), actions = states["m"], states["state"], states["actions"]
    # the oracle on the handle's own numbers: its model (per-env dynamics: each state's row applied to it) and the task it runs
    task = sim.get_task()
    b = oracle.Batch(sim.model, task, m)
    b.set_state(q.astype(np.float64), v.astype(np.float64), a.astype(np.float64), None, ns)
    obs_o, rew_o, done_o, _ = b.step(actions.astype(np.float64))
    q_o, v_o, a_o, _, n_o = b.get_state()
    if leaf.dyn:
        obs_o, rew_o, _, q_o, v_o, a_o = oracle_per_env(oracle, sim.model, task, states["rows"], states["state"], actions)
    tail_ok = ~done_o
    chain = None
    if env is not None:
        chain = chains(leaf.robot, leaf.dyn, sim.model, task)
        tail_ok = tail_ok & ~chain["outs"][0]["done"] & ~chain["outs"][1]["done"]
    # a plain step does not restart an env that finishes, and compares it: there every touching state may be a block's contact env (a
    # robot with its FRAME on the floor is below the fall height); the walking and PO layers restart it, so theirs must not terminate
    idx = layout(n, m, states["touch"], tail_ok, block_ok=np.ones(m, bool) if env is None else tail_ok)
    in_block = np.unique(idx[m:][states["touch"][idx[m:]]]) if n > m else np.zeros(0, np.int64)
    if "built" in states and n > m:
        # the second pool: which built states are the one touching env of a block in this leaf
        may = states["built"] if env is None else states["built"][tail_ok[states["built"]]]
        if env is not None:
            assert tail_ok[states["built"][states["upright"]]].all(), "a built state that stands upright ends no walking episode"
        slots = int((states["touch"][idx[m:]]).sum())
        assert np.array_equal(in_block, may[:min(slots, len(may))]) and len(in_block) >= min(slots, int(states["upright"].sum()))
        lab = states["label"][np.searchsorted(states["built"], in_block)]
        print(f"{name} n={n}: {len(in_block)} of {len(states['built'])} built states sit alone in a block ({slots} blocks): "
              f"{int((lab[:, 0] == CC.KIND_EDGE).sum())} cull-edge, {int(((lab[:, 0] == CC.KIND_CELL) & (lab[:, 1] == 0)).sum())} FRAME points, "
              f"{int(((lab[:, 0] == CC.KIND_CELL) & (lab[:, 1] > 0)).sum())} femur points")
    if env is not None:
        first = env.reset()
        env.set_commands(states["velocity"][idx], states["heading"][idx])
    if leaf.dyn:
        sim.set_dynamics(states["rows"][idx])
    sim.set_state(q[idx], v[idx], a[idx], None, ns[idx])
    if env is None:
        obs, rew, done, _ = sim.step(actions[idx])
    else:
        obs, rew, done, _ = env.step(actions[idx])
        comps = env.last_components.copy()
    assert sim.last_step_kernel == name
    q1, v1, a1, _, n1 = sim.get_state()
    if n > m:                                                   # every state sits once at the front: env e < m holds state e
        assert np.array_equal(idx[:m], np.arange(m))
        same_bits_wherever_it_sits(idx, states["touch"], m, np.zeros(n, bool) if env is None else done,
                                   dict(qpos=q1, qvel=v1, act=a1, nstep=n1, obs=obs, reward=rew, done=np.asarray(done, bool)))
    if env is not None:
        # the second env-step: the same states again (the task layers keep their histories), other actions
        sim.set_state(q[idx], v[idx], a[idx], None, ns[idx])
        obs2, rew2, done2, _ = env.step(states["actions2"][idx])
        comps2 = env.last_components.copy()
        assert sim.last_step_kernel == name
        env.close()
    else:
        sim.close()
    keep = np.ones(n, bool) if env is None else ~np.asarray(done, bool)     # walking / PO: finished envs were auto-reset
    if n > 4 * TAIL:
        assert keep[-TAIL:].all(), "the tail (the last, partial workgroup) is compared"
    assert keep.sum() >= min(n, m) // 2
    j = idx[keep]
    t = TOL["A"]
    close(q1[keep], q_o[j], t["qpos"], "qpos")
    close(v1[keep], v_o[j], t["qvel"], "qvel")
    close(a1[keep], a_o[j], t["act"], "act")
    assert np.array_equal(n1[keep], n_o[j])
    if leaf.layer != "po":
        obs = np.asarray(obs)[keep]
        mask = np.ones(obs.shape[1], bool)
        mask[12:15] = False
        close(obs[:, mask], obs_o[j][:, mask], t["obs"], "obs")
        close(obs[:, 12:15], obs_o[j][:, 12:15], t["accel"], "accelerometer")
    if leaf.layer == "none":
        close(rew, rew_o[idx], t["reward"], "reward")
        if not leaf.dyn:
            sure = np.abs(q_o[idx, 2] - 0.05) > 1e-4
            assert np.array_equal(np.asarray(done, bool)[sure], done_o[idx][sure])
    if env is None:
        return
    # ---- walking and PO leaves: rewards, and the whole stack, against the composed checker (tests/po_step_reference.py) -----------
    # Reward components: the f32 reward against the f64 one on equal sensors is held to 2e-4 / 2e-4 (component 10: its own formula)
    # by test_walking_rewards_match_oracle; here the sensors are the ORACLE's, so each component may also move by its sensitivity to
    # sensors that differ within TOL["A"], measured on the oracle alone (fixture `chains`: 8 seeded sign patterns, largest change
    # over the states, per step).
    # Euler angles (R.angle_bound): 2e-4, the bound of test_po_frames_match_oracle for the f32 filter on EQUAL inputs, plus
    # 2 * GAIN_IMU * dt -- the filter's correction is a step of length gain * dt along the UNIT gradient, whose direction is
    # discontinuous in the accelerometer input where the estimate is aligned with gravity, so an accelerometer reading within its
    # tolerance can turn that step around -- plus dt * (atol + rtol * |gyro|), the gyro's obs tolerance integrated over the step.
    # Everything else of a frame: gyro and body velocity TOL obs, accelerometer TOL accel, ctrl and command 1e-6 (exact values in
    # f32); the frames behind the computed ones are the reset frame, exact values only.
    both = keep & ~np.asarray(done2, bool)
    if n > 4 * TAIL:
        assert both[-TAIL:].all(), "the tail (the last, partial workgroup) is compared in the second step too"
    assert both.sum() >= min(n, m) // 2
    maxima = {}
    dt = chain["dt"]
    steps = ((keep, obs, rew, comps), (both, obs2, rew2, comps2))
    for s, (sel, o_s, r_s, c_s) in enumerate(steps):
        exp, rows, js = chain["outs"][s], np.flatnonzero(sel), idx[sel]
        what = f"step {s + 1}"
        R.compare_rewards(c_s[sel], np.asarray(r_s)[sel], exp["comps"][js], exp["reward"][js], chain["sensitivity"][s], dt,
                          what + " reward", rows=rows, maxima=maxima, sens=exp["sens"][js], tol=t)
        if leaf.layer == "po":
            R.compare_stack(np.asarray(o_s)[sel], exp["stack"][js], t, dt, computed=s + 1, what=what + " stack", rows=rows, maxima=maxima)
    if leaf.layer == "po":
        assert np.allclose(first, chain["reset"][idx], rtol=0, atol=R.EXACT), "the stack reset() returns"
    R.record(RECORD, f"{name} pool={states['pool']} n={n} compared={int(keep.sum())}/{int(both.sum())}\n    " + R.format_maxima(maxima))
