"""The one-step floating-point contract of the step kernels, and the few names every parity test shares.

The kernels compute in f32, the oracle in f64; the tolerances are stated per quantity below and hold for ONE env-step from identical
f32 states (longer rollouts diverge chaotically in any precision and are compared through invariants instead).  Nothing in here
touches the GPU or imports torch at import: the CPU censuses and tools/make_contact_cells.py read the same numbers."""
import os

import numpy as np
import pytest

from quadruped_gym_amd import _abi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_vectors.npz")
MAPPINGS = {"lane": _abi.MAP_LANE, "quad": _abi.MAP_QUAD, "pair": _abi.MAP_PAIR, "link": _abi.MAP_LINK}

# ---- stated tolerances: |gpu - oracle| <= atol + rtol * |oracle| after one env-step ----------
# The absolute terms are <= 5x the largest error MEASURED over 4096 seeded states per frame_skip and every work mapping
# (tools/parity_report.py -> profiles/r02/parity_report.txt; frame_skip 4: qpos 1.2e-6, qvel 4.3e-4, act 8.2e-8, obs 7.5e-5,
# accelerometer 5.3e-3 m/s^2, reward 3.5e-6), so a regression that costs an order of magnitude of accuracy fails.  frame_skip
# 20 compounds 20 substeps and a contact can switch inside the step (measured maxima qpos 1.5e-4, qvel 7.7e-2, obs 5.8e-4,
# accelerometer 0.85, reward 3.0e-4).
TOL = {
    "A": dict(qpos=(5e-6, 2e-6), qvel=(2e-3, 1e-4), act=(4e-7, 1e-6), obs=(3.5e-4, 1e-4), accel=(0.025, 1e-3), reward=(1.5e-5, 1e-5)),
    "B": dict(qpos=(4e-4, 1e-4), qvel=(5e-2, 2e-2), act=(6e-7, 1e-6), obs=(3e-3, 2e-3), accel=(2.0, 5e-2), reward=(1.5e-3, 1e-3)),
}
# frame_skip 20, accelerometer (round 4): the 2.0 m/s^2 above is set by the handful of states where a contact switches inside the
# step -- a body touches down or lifts off at a slightly different substep in f32 and the reading of the last substep jumps.  States
# whose contact census (the oracle's contact_W > 0 per body) does NOT change around the substep the sensors describe (the last one and
# two before it, one after: oracle.contact_switch_near_sensors) are held to this bound instead; the loose one only covers the rest.
ACCEL_B_STEADY = (0.01, 1e-3)        # measured: 4.2e-4 on the golden states (every mapping), 1.7e-3 on config 5's 4096-env sample


def close_accel_b(oracle, got, ref, model, frame_skip, state, actions, keep=None):
    qpos, qvel, act, nstep = state
    changed = oracle.contact_switch_near_sensors(model, frame_skip, qpos, qvel, act, nstep, actions)
    if keep is not None:
        got, ref, changed = got[keep], ref[keep], changed[keep]
    steady = ~changed
    assert steady.sum() >= 20, "enough states keep their contacts around the sensor substep"
    worst = close(got[steady], ref[steady], ACCEL_B_STEADY, "accelerometer (contact census steady)")
    if changed.any():
        close(got[changed], ref[changed], TOL["B"]["accel"], "accelerometer (a contact switches inside the step)")
    return worst, int(changed.sum())


def configure(task, case):
    task.use_fall = 1
    task.fall_height = 0.05
    if case == "B":
        task.frame_skip = 20
        task.obs_mode = 1
    return task


def close(got, ref, tol, what):
    atol, rtol = tol
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = atol + rtol * np.abs(ref)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert (err <= bound).all(), f"{what}: max excess at {worst}: got {np.asarray(got)[worst]}, ref {ref[worst]}, err {err[worst]:.3e}"
    return float(err.max())


def accel_slice(case):
    return slice(12, 15)


def simds():
    """SIMDs of device 0 (1024 on an MI355X): the step kernels' AUTO boundaries are "one wave per SIMD" sizes."""
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))
