"""Seeded auto-resetting rollouts of the step kernels, recorded once and replayed bit for bit.

``FORMS`` names one rollout per step-kernel instantiation whose prologue / epilogue text is shared (every one-link-per-lane
kernel, and the one-leg-per-lane kernel where it is alone on its SIMD).  ``rollout(form, robot_dir)`` runs it on the GPU and returns
the arrays a recording keeps: the LAST env-step's outputs and the final ``qpos / qvel / act / ctrl / nstep`` of the first ``KEEP``
envs, plus how many of them were reset on the way.  tools/record_rollouts.py writes them to tests/golden/rollouts/<form>.npz (from
the build whose bits are to be kept); tests/test_rollout_bits_gpu.py replays them against the current build.

The rollout: STEPS env-steps of frame_skip 4 from a reset, actions ``default_rng(7).uniform(-1, 1)``, fall termination at 0.05 m,
auto-reset with a random yaw -- a few of 256 envs fall within 40 env-steps (none in the first 10), so every recording crosses
the reset path of its kernel."""
import contextlib
import os
from dataclasses import dataclass

import numpy as np

from quadruped_gym_amd import _abi

from helpers import write_table_robot
from kernel_leaves import PO_WINDOW, open_leaf

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "rollouts")
STEPS, KEEP, SEED, ACTION_SEED, FALL_HEIGHT = 40, 256, 3, 7, 0.05


@dataclass(frozen=True)
class Form:
    kernel: str             # what BatchedSim.last_step_kernel must report
    n: int = 256
    robot: str = "baked"    # "baked": the compiled-in robot; "table": a slightly modified one (table-driven kernels)
    layer: str = "none"     # "none" (plain step, packed rows), "walk", "po"
    dyn: bool = False       # identity per-env dynamics rows: the DYN instantiation on the shared model's numbers
    helpers: bool = True    # QG_LINK_HELPERS at qg_create
    mapping: str = "auto"   # every recording runs the mapping AUTO picks at its size


FORMS = {
    "plain": Form("qg_step_kernel_link<0,0,1,0,0>"),
    "walk": Form("qg_step_kernel_link<1,0,1,1,0>", layer="walk"),
    "walk_one_role": Form("qg_step_kernel_link<1,0,1,0,0>", layer="walk", helpers=False),
    "po": Form("qg_step_kernel_link<1,1,1,1,0>", layer="po"),
    "po_one_role": Form("qg_step_kernel_link<1,1,1,0,0>", layer="po", helpers=False),
    "table_plain": Form("qg_step_kernel_link<0,0,0,0,0>", robot="table"),
    "table_walk": Form("qg_step_kernel_link<1,0,0,0,0>", robot="table", layer="walk"),
    "table_po": Form("qg_step_kernel_link<1,1,0,0,0>", robot="table", layer="po"),
    "dyn_plain": Form("qg_step_kernel_link<0,0,0,0,1>", dyn=True),
    "dyn_walk": Form("qg_step_kernel_link<1,0,0,0,1>", layer="walk", dyn=True),
    "dyn_po": Form("qg_step_kernel_link<1,1,0,0,1>", layer="po", dyn=True),
    "quad_8192": Form("qg_step_kernel_quad<1,1,0,4,0,0,0>", n=8192),
    "pair_32768": Form("qg_step_kernel_pair<4,0,0>", n=32768),
}


def _task(task):
    task.use_fall, task.fall_height = 1, FALL_HEIGHT
    task.auto_reset, task.reset_flags = 1, _abi.RESET_RANDOM_YAW
    return task


@contextlib.contextmanager
def _falling_walkers():
    """The walking VecEnvs build their task themselves (flip + time limit); the rollouts want the fall termination on top."""
    from quadruped_gym_amd.envs import walking
    real = walking.BatchedSim

    def with_fall(n, **kw):
        kw["task"] = _task(kw["task"])
        return real(n, **kw)
    walking.BatchedSim = with_fall
    try:
        yield
    finally:
        walking.BatchedSim = real


def rollout(form: Form, robot_dir):
    from quadruped_gym_amd.model.loader import load_model
    n = form.n
    table = None
    if form.robot == "table":
        path = write_table_robot(robot_dir)
        table = (path, load_model(path)[0])
    with _falling_walkers():
        sim, env = open_leaf(form, n, table, auto_reset=True, reset_flags=_abi.RESET_RANDOM_YAW, seed=SEED, obs_window=PO_WINDOW,
                             random_init=True)
    if env is None:
        sim.reset(seed=SEED, flags=_abi.RESET_RANDOM_YAW)
    else:
        env.reset()
    if form.dyn:
        sim.set_dynamics(np.tile(_abi.identity_dynamics_row(sim.model), (n, 1)).astype(np.float32))
    assert sim.baked == (form.robot == "baked" and not form.dyn)
    actions = np.random.default_rng(ACTION_SEED).uniform(-1, 1, (STEPS, n, 12)).astype(np.float32)
    resets = np.zeros(n, np.int32)
    out = {}
    for t in range(STEPS):
        if env is None:             # the packed row (obs, reward, done): the form a throughput loop runs
            import torch
            packed = torch.empty((n, sim.obs_dim + 2), dtype=torch.float32, device=f"cuda:{sim.device}")
            sim.step_device_packed(torch.from_numpy(actions[t]).to(packed.device), packed)
            out = {"packed": packed.cpu().numpy()}
            done = out["packed"][:, -1] != 0.0
        else:
            obs, rew, done, _ = env.step(actions[t])
            out = {"obs": np.asarray(obs), "reward": rew, "done": np.asarray(done).astype(np.uint8), "components": env.last_components}
        resets += np.asarray(done, bool)
    kernel = sim.last_step_kernel
    qpos, qvel, act, ctrl, nstep = sim.get_state()
    out.update(qpos=qpos, qvel=qvel, act=act, ctrl=ctrl, nstep=nstep, resets=resets)
    if env is not None:
        f_est, a_est, ideal = env.estimates()
        out.update(f_est=f_est, a_est=a_est, ideal=ideal)
        env.close()
    else:
        sim.close()
    assert kernel == form.kernel, (kernel, form.kernel)
    return {k: np.ascontiguousarray(v[:KEEP]) for k, v in out.items()}


def golden_path(name):
    return os.path.join(GOLDEN, name + ".npz")
