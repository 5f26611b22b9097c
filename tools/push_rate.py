"""Cost of external wrenches: microseconds per step launch (qg_time_step_kernel, frame_skip 4) at 4096 (LINK), 16 384 and 32 768 (QUAD)
envs of the compiled-in robot, for
  dyn       the per-env-dynamics kernel with identity rows, wrench mode off (the baseline of this table)
  zero      wrench mode on, every row zero
  random    wrench mode on, random forces and torques on every body
  push      wrench mode on, zero rows and the push schedule (interval 3, duration 2, probability 0.6)
Rounds alternate the four forms (same GPU, same process); prints the median of each and the wrench forms' cost over `dyn`.
usage: python tools/push_rate.py [rounds] [iters]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quadruped_gym_amd import _abi  # noqa: E402
from quadruped_gym_amd.sim import BatchedSim  # noqa: E402

FORMS = ("dyn", "zero", "random", "push")


def make(form, n):
    model = _abi.default_model()
    task = _abi.default_task()
    task.auto_reset = 1
    sim = BatchedSim(n, model=model, task=task)
    sim.set_dynamics(np.tile(_abi.identity_dynamics_row(model), (n, 1)))
    if form == "zero":
        sim.set_external_wrench(np.zeros((n, 13, 6), np.float32))
    elif form == "random":
        rows = np.random.default_rng(1).uniform(-0.5, 0.5, (n, 13, 6)).astype(np.float32)
        rows[:, :, 3:6] *= 0.01
        sim.set_external_wrench(rows)
    elif form == "push":
        sim.set_push_schedule({"interval": 3, "duration": 2, "probability": 0.6, "force": (1.0, 3.0)})
    sim.reset(seed=1, flags=_abi.RESET_RANDOM_YAW)
    sim.set_track_ctrl(False)
    return sim


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    dev = torch.device("cuda:0")
    print(f"build {_abi.load_library().qg_build_id().decode()}; frame_skip 4, {iters} launches per sample, {rounds} alternated rounds")
    for n in (4096, 16384, 32768):
        sims = {f: make(f, n) for f in FORMS}
        acts = torch.rand((n, 12), device=dev) * 2 - 1
        packed = torch.empty((n, 35), device=dev)
        for s in sims.values():
            s.time_step_kernel(acts, packed, 50)         # warm-up
        t = {f: [] for f in FORMS}
        for _ in range(rounds):
            for f in FORMS:
                t[f].append(sims[f].time_step_kernel(acts, packed, iters) * 1e3)
        med = {f: float(np.median(v)) for f, v in t.items()}
        maps = {f: {_abi.MAP_LINK: "link", _abi.MAP_QUAD: "quad"}.get(sims[f].mapping, "?") for f in FORMS}
        kern = {sims[f].last_step_kernel for f in FORMS}
        assert len(kern) == 1, kern
        line = "  ".join(f"{f} {med[f]:6.2f} us ({maps[f]})" for f in FORMS)
        over = "  ".join(f"{f} {100 * (med[f] / med['dyn'] - 1):+.1f} %" for f in FORMS[1:])
        spread = "  ".join(f"{f} {min(t[f]):.2f}-{max(t[f]):.2f}" for f in FORMS)
        print(f"{n:6d} envs: {line}   [{kern.pop()}]")
        print(f"{'':12s}over dyn: {over};  round range (us): {spread}")
        for s in sims.values():
            s.close()


if __name__ == "__main__":
    main()
