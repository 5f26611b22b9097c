"""Step-kernel time where auto-resets are the norm: microseconds per launch (qg_time_step_kernel) at 4096 envs of the compiled-in robot
on bench.py's task (frame_skip 4, fall termination at 0.05 m, auto-reset, data.ctrl tracked), with the time limit at LIMIT env-steps
and the envs' clocks staggered over it before timing, so that 1 / LIMIT of the envs (about 1 %) restart in EVERY launch -- the phase
of a training run whose episodes are out of step, which the headline (every env in phase, 1250 env-steps to the limit) does not show.
`inphase` is the same task with every clock at zero: no time-limit reset inside the timed launches.
One library per process (QUADGYM_LIB); alternate the builds from the shell:
  for r in 1 2 3 4; do for L in libA.so libB.so; do QUADGYM_LIB=$L python tools/reset_rate.py; done; done
usage: python tools/reset_rate.py [--random-yaw] [--samples S] [--iters I]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quadruped_gym_amd import _abi  # noqa: E402
from quadruped_gym_amd.sim import BatchedSim  # noqa: E402

N, LIMIT = 4096, 100


def make(staggered, yaw):
    task = _abi.default_task()
    task.frame_skip, task.use_fall, task.fall_height, task.auto_reset = 4, 1, 0.05, 1
    task.reset_flags = _abi.RESET_RANDOM_YAW if yaw else 0
    task.max_time = LIMIT * task.frame_skip * _abi.default_model().timestep
    sim = BatchedSim(N, task=task)
    assert sim.limit_substeps == LIMIT * task.frame_skip, sim.limit_substeps
    sim.set_track_ctrl(True)
    sim.reset(seed=0, flags=task.reset_flags)
    if staggered:
        sim.set_state(nstep=(task.frame_skip * (np.arange(N) % LIMIT)).astype(np.int32))
    return sim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--random-yaw", action="store_true")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--iters", type=int, default=400)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    acts = torch.rand((N, 12), device=dev) * 2 - 1
    packed = torch.empty((N, 35), device=dev)
    out = []
    for name, staggered in (("inphase", False), ("staggered", True)):
        sim = make(staggered, args.random_yaw)
        sim.time_step_kernel(acts, packed, 100)                 # warm-up (a multiple of LIMIT: the stagger stays as set)
        ep0 = sim.get_reset_streams()[0].astype(np.int64).sum()
        t = [sim.time_step_kernel(acts, packed, args.iters) * 1e3 for _ in range(args.samples)]
        resets = (sim.get_reset_streams()[0].astype(np.int64).sum() - ep0) / (args.samples * args.iters)
        kern = sim.last_step_kernel
        sim.close()
        out.append(f"{name} {np.median(t):6.3f} us (range {min(t):.3f}-{max(t):.3f}, {resets:5.1f} resets/launch)")
    lib = os.path.basename(os.environ.get("QUADGYM_LIB", "libquadgym.so"))
    print(f"{lib:28s} build {_abi.load_library().qg_build_id().decode()}  {'yaw ' if args.random_yaw else ''}" + "  ".join(out) + f"  [{kern}]")


if __name__ == "__main__":
    main()
