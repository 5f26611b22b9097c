"""What ContactSensor.read (one launch: csrc/qg_contact.hip) costs at 4096 and 32 768 envs, and what it adds to the env-step it rides
behind.

  read:       sensor.read(done, body_force=..., feet=...)            forces of 13 bodies, four foot rows, timers advanced
  step:       sim.step_device_packed(actions, packed)                the env-step alone
  step+read:  the two launches, the read taking the step's done column

Each side is timed eagerly (host clock around `reps` calls that end in a synchronise) and as a hipGraph of one call (torch.cuda.graph),
all sides in alternating rounds in this one process on the same build; the median of the rounds is reported with their spread
(max - min).  The robots stand on the floor (a settled rollout), so every foot lane runs the whole contact law.

usage (GPU box): python tools/contact_sensor_rate.py [--rounds 7] [--reps 1000] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.contact import ContactSensor
from quadruped_gym_amd.sim import BatchedSim

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=1000)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
SIZES = (4096, 32768)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def time_sides(sides):
    """``{(mode, name): (median us/call, spread)}`` of the callables ``sides``, eagerly and as a graph of one call."""
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        for fn in sides.values():
            for _ in range(3):
                fn()
    side.synchronize()
    graphs = {}
    for name, fn in sides.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn()
        graphs[name] = g
    result = {}
    for mode in ("eager", "graph"):
        calls = {name: (graphs[name].replay if mode == "graph" else sides[name]) for name in sides}
        times = {name: [] for name in sides}
        with torch.cuda.stream(side):
            for call in calls.values():
                for _ in range(20):
                    call()
            side.synchronize()
            for _ in range(args.rounds):
                for name, call in calls.items():         # alternated: one round of each in turn
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        call()
                    side.synchronize()
                    times[name].append((time.perf_counter() - t0) / args.reps * 1e6)
        for name, ts in times.items():
            result[(mode, name)] = (statistics.median(ts), max(ts) - min(ts))
    del graphs
    return result


def measure(n):
    task = _abi.default_task()
    task.auto_reset = 1
    sim = BatchedSim(n, task=task)
    sim.reset(seed=1)
    sensor = ContactSensor(sim)
    actions = torch.tensor([0.0, 0.0, -0.5] * 4, device=dev).repeat(n, 1).contiguous()
    packed = torch.zeros((n, sim.obs_dim + 2), device=dev)
    force, feet = torch.empty((n, 13, 3), device=dev), torch.empty((n, 4, 12), device=dev)
    for _ in range(150):                                     # the robots settle on their feet
        sim.step_device_packed(actions, packed)
    sensor.read(body_force=force, feet=feet)
    torch.cuda.synchronize()
    standing = float((feet[:, :, 6].sum(1) > 0).float().mean())
    done = packed[:, sim.obs_dim + 1]

    def read():
        sensor.read(done=done, body_force=force, feet=feet)

    def step():
        sim.step_device_packed(actions, packed)

    def both():
        sim.step_device_packed(actions, packed)
        sensor.read(done=done, body_force=force, feet=feet)

    result = time_sides({"read": read, "step": step, "step+read": both})
    for mode in ("eager", "graph"):
        r, s, b = result[(mode, "read")], result[(mode, "step")], result[(mode, "step+read")]
        say(f"{n:6d} envs  {mode:5s}: read {r[0]:6.1f} (spread {r[1]:4.1f})   step {s[0]:6.1f} (spread {s[1]:4.1f})   step+read {b[0]:6.1f} "
            f"(spread {b[1]:4.1f}) us   the read adds {b[0] - s[0]:5.1f} us = {100.0 * (b[0] - s[0]) / s[0]:4.0f} % of the step   "
            f"[{sim.last_step_kernel}; {100 * standing:.0f} % of the robots on their feet]")
    sensor.close()
    sim.close()


say(f"# tools/contact_sensor_rate.py: {args.rounds} alternated rounds of {args.reps} calls, median us per call; build "
    f"{_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
for n in SIZES:
    measure(n)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
