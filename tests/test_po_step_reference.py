"""The composed walking / PO checker (tests/po_step_reference.py) and the comparisons the GPU tests apply with it, on the CPU.

Run on the states, actions and commands of the leaf tests (tests/leaf_states.py: ``build_states``), with the two env-steps the walking and
PO leaves take: the comparisons pass on the checker's own frames (rounded to f32, and rebuilt from sensors moved within the one-step
parity tolerance), and fail for each of eight deliberate miswirings of a step kernel's gather -- so the chosen states and the stated
tolerances separate those mistakes."""
import numpy as np
import pytest

import po_step_reference as R
from leaf_states import PO_WINDOW, build_states, expected_chain, walking_task
from parity import TOL

T = TOL["A"]


@pytest.fixture(scope="module")
def leaf(oracle):
    """What a PO leaf of the compiled-in robot is compared with, and the un-lagged sensors of the first step."""
    st = build_states(oracle)
    model, task = oracle.default_model(), walking_task()
    chain = expected_chain(oracle, st, model, task, dyn=False)
    applied, _ = R.gated_control(st["state"][3], st["actions"], 0.0)
    unlagged = R.physics(oracle, model, task, st["state"], applied, unlagged=True)
    assert np.array_equal(unlagged["sens"], chain["outs"][0]["sens"])
    keep = ~chain["outs"][0]["done"] & ~chain["outs"][1]["done"]
    assert keep.sum() >= st["m"] // 2
    for k, row in enumerate(chain["sensitivity"]):
        print(f"reward sensitivity, step {k + 1}: " + " ".join(f"{x:.3e}" for x in row))
    return dict(st=st, chain=chain, keep=keep, unlagged=unlagged["sens_unlagged"], model=model, task=task)


def device_like(leaf):
    """What a correct kernel would return for the two steps: the checker's numbers in f32, kept envs only."""
    keep = leaf["keep"]
    return [dict(stack=o["stack"][keep].astype(np.float32).astype(np.float64), comps=o["comps"][keep].astype(np.float32).astype(np.float64),
                 reward=o["comps"][keep].astype(np.float32).sum(1, dtype=np.float32).astype(np.float64)) for o in leaf["chain"]["outs"]]


def compare(leaf, got):
    """The leaf test's comparison of both steps."""
    chain, keep = leaf["chain"], leaf["keep"]
    maxima = {}
    for s, (g, exp) in enumerate(zip(got, chain["outs"])):
        R.compare_rewards(g["comps"], g["reward"], exp["comps"][keep], exp["reward"][keep], chain["sensitivity"][s], chain["dt"],
                          f"step {s + 1} reward", maxima=maxima, sens=exp["sens"][keep], tol=T)
        R.compare_stack(g["stack"].reshape(len(g["stack"]), -1), exp["stack"][keep], T, chain["dt"], computed=s + 1,
                        what=f"step {s + 1} stack", maxima=maxima)
    return maxima


def test_reset_stack_and_fifo_of_the_checker(leaf):
    chain, st = leaf["chain"], leaf["st"]
    reset = chain["reset"].reshape(st["m"], PO_WINDOW, R.FRAME)
    assert not reset[:, :, :11].any() and not reset[:, :, 23:].any()            # zero sensors, angles of [1,0,0,0], no command yet
    assert np.array_equal(reset[:, :, 11:23], np.tile(R.DEFAULT_CTRL, (st["m"], PO_WINDOW, 1)))
    s1, s2 = chain["outs"][0]["stack"], chain["outs"][1]["stack"]
    assert np.array_equal(s1[:, :2], reset[:, 1:]) and np.array_equal(s2[:, 0], reset[:, 2]) and np.array_equal(s2[:, 1], s1[:, 2])
    # the second step's actions reach beyond the clip, its data.ctrl does not; the command shows from the first step on
    assert (np.abs(st["actions2"]) > 1).any(1).mean() > 0.5 and np.abs(s2[:, 2, 11:23]).max() == 1.0
    assert np.allclose(s1[:, 2, 23:25], st["velocity"]) and np.abs(s1[:, 2, 25]).max() > 3.0
    # component 10 is zero on the first step after a reset (no previous value) and alive on the second
    assert not chain["outs"][0]["comps"][:, 10].any() and np.abs(chain["outs"][1]["comps"][:, 10]).max() > 5.0
    assert np.isfinite(chain["sensitivity"]).all() and not chain["sensitivity"][0, 10]


def test_the_checkers_own_frames_pass(leaf):
    maxima = compare(leaf, device_like(leaf))
    print(R.format_maxima(maxima))
    assert max(v for k, v in maxima.items() if k != R.RATIOS) < 1e-4                                           # f32 rounding only (the total: an f32 sum of eleven)


def test_frames_from_sensors_within_tolerance_pass(leaf, oracle):
    """The derived bounds hold together: a chain whose task oracles see sensors moved by up to the one-step parity tolerance (what a
    correct f32 kernel may show) passes the comparison with the unmoved chain."""
    st, chain, keep = leaf["st"], leaf["chain"], leaf["keep"]
    chk = R.StepChecker(oracle, st["m"], leaf["task"].frame_skip, obs_window=PO_WINDOW)
    chk.reset()
    chk.set_commands(st["velocity"], st["heading"])
    rng = np.random.default_rng(5)
    got = []
    for s, actions in enumerate((st["actions"], st["actions2"])):
        sens = chain["outs"][s]["sens"]
        o = chk.step(leaf["model"], leaf["task"], st["state"], actions, perturb=rng.uniform(-1, 1, sens.shape) * R.sensor_bound(sens, T))
        got.append(dict(stack=o["stack"][keep], comps=o["comps"][keep], reward=o["comps"][keep].sum(1)))
    print(R.format_maxima(compare(leaf, got)))


def _swap_gyro_accel(leaf, got):
    f = got[0]["stack"][:, -1]
    f[:, 0:3], f[:, 3:6] = f[:, 3:6].copy(), f[:, 0:3].copy()


def _body_velocity_from_the_z_axis(leaf, got):
    got[0]["stack"][:, -1, 9:11] = leaf["chain"]["outs"][0]["sens"][leaf["keep"], 27:29]


def _no_sensor_lag(leaf, got):
    s = leaf["unlagged"][leaf["keep"]]
    f = got[0]["stack"][:, -1]
    f[:, 0:3], f[:, 3:6], f[:, 9:11] = s[:, 15:18], s[:, 12:15], s[:, 30:32]


def _ctrl_not_clipped(leaf, got):
    got[1]["stack"][:, -1, 11:23] = leaf["chain"]["outs"][1]["applied"][leaf["keep"]]


def _neighbours_frame(leaf, got):
    got[0]["stack"][:, -1] = np.roll(got[0]["stack"][:, -1], -1, axis=0)


def _newest_frame_first(leaf, got):
    got[0]["stack"] = np.roll(got[0]["stack"], 1, axis=1)


def _angles_before_the_update(leaf, got):
    got[1]["stack"][:, -1, 6:9] = leaf["chain"]["outs"][1]["pre_angles"][leaf["keep"]]


def _component_10_with_another_dt(leaf, got):
    c = got[1]["comps"]
    c[:, 10] *= leaf["task"].frame_skip / 10.0                                   # divided by the dt of frame_skip 10
    got[1]["reward"] = c.astype(np.float32).sum(1, dtype=np.float32).astype(np.float64)


MISWIRINGS = [(_swap_gyro_accel, "step 1 stack newest (gyro|accel)"), (_body_velocity_from_the_z_axis, "step 1 stack newest body_vel"),
              (_no_sensor_lag, "step 1 stack newest (gyro|accel|body_vel)"), (_ctrl_not_clipped, "step 2 stack newest ctrl"),
              (_neighbours_frame, "step 1 stack newest"), (_newest_frame_first, "step 1 stack"),
              (_angles_before_the_update, "step 2 stack newest angles"), (_component_10_with_another_dt, "step 2 reward component 10")]


@pytest.mark.parametrize("miswire,where", MISWIRINGS, ids=[f.__name__[1:] for f, _ in MISWIRINGS])
def test_miswiring_is_detected(leaf, miswire, where):
    got = device_like(leaf)
    miswire(leaf, got)
    with pytest.raises(AssertionError, match=where):
        compare(leaf, got)


def test_history_free_columns_equal_the_chains(leaf, oracle):
    """``gated_control`` + ``physics`` + ``frame_columns`` (what the rollout test of tests/test_po_env.py restarts from the device's state
    at every step) give the chain's newest frame outside the angle columns, and the settling gate replaces the action before the clip."""
    st, out = leaf["st"], leaf["chain"]["outs"][1]
    applied, ctrl = R.gated_control(st["state"][3], st["actions2"], 0.0)
    fr = R.frame_columns(R.physics(oracle, leaf["model"], leaf["task"], st["state"], applied)["sens"], ctrl, st["velocity"], st["heading"])
    cols = np.r_[0:6, 9:26]
    assert np.array_equal(fr[:, cols], out["stack"][:, -1, cols]) and np.isnan(fr[:, 6:9]).all()
    ns = np.array([0, 39, 40, 41], np.int32)                                      # 0.08 s = 40 substeps on the f64 clock
    applied, ctrl = R.gated_control(ns, np.full((4, 12), 1.2), 0.08)
    assert np.array_equal(applied[:, 0], [0.0, 0.0, 1.2, 1.2]) and np.array_equal(ctrl[:, 2], [-0.5, -0.5, 1.0, 1.0])
