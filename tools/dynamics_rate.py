"""Cost of per-env dynamics: microseconds per step launch (qg_time_step_kernel, frame_skip 4) at 4096, 16 384 and 32 768 envs for
  generic   the table-driven kernel on a tweaked robot (act_kp x 1.1)
  identity  the same robot, per-env mode with identity rows
  random    the same robot, per-env mode with rows drawn from a wide range
  baked     the compiled-in robot (literal-constant kernel)
  dyn-dflt  the compiled-in robot, per-env mode with random rows
Rounds alternate the five forms (same GPU, same process); prints the median of each and the per-env forms' cost over `generic`.
usage: python tools/dynamics_rate.py [rounds] [iters]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quadruped_gym_amd import _abi  # noqa: E402
from quadruped_gym_amd.sim import BatchedSim  # noqa: E402

WIDE = {"friction": (0.3, 1.5), "payload_mass": (-0.1, 0.3), "payload_pos": ((-0.015, 0.015),) * 3, "kp_scale": (0.6, 1.4),
        "kv_scale": (0.6, 1.4), "force_scale": (0.6, 1.4), "damping_scale": (0.6, 1.4), "contact_stiffness_scale": (0.5, 2.0),
        "contact_damping_scale": (0.5, 2.0)}
FORMS = ("generic", "identity", "random", "baked", "dyn-dflt")


def make(form, n):
    model = _abi.default_model()
    if form in ("generic", "identity", "random"):
        for j in range(12):
            model.act_kp[j] *= 1.1
    task = _abi.default_task()
    task.auto_reset = 1
    sim = BatchedSim(n, model=model, task=task)
    if form == "identity":
        sim.set_dynamics(np.tile(_abi.identity_dynamics_row(model), (n, 1)))
    elif form in ("random", "dyn-dflt"):
        sim.set_dynamics_range(WIDE)
        sim.reset(seed=1, flags=_abi.RESET_DYNAMICS)
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
        maps = {f: {_abi.MAP_LINK: "link", _abi.MAP_QUAD: "quad", _abi.MAP_PAIR: "pair"}.get(sims[f].mapping, "?") for f in FORMS}
        line = "  ".join(f"{f} {med[f]:6.2f} us ({maps[f]})" for f in FORMS)
        over = "  ".join(f"{f} {100 * (med[f] / med['generic'] - 1):+.1f} %" for f in ("identity", "random"))
        print(f"{n:6d} envs: {line}")
        print(f"{'':12s}per-env over generic: {over};  dyn-dflt over baked {100 * (med['dyn-dflt'] / med['baked'] - 1):+.1f} %;"
              f"  M env-steps/s: generic {n / med['generic']:.0f}, random {n / med['random']:.0f}")
        for s in sims.values():
            s.close()


if __name__ == "__main__":
    main()
