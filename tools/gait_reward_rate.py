"""What the gait-shaped reward terms cost behind the env-step at 4096 and 32 768 envs: the fused launch (csrc/qg_gait.hip) against
sensor.read followed by the closest torch expression of the seven terms and the reward add.

  step:             sim.step_device_packed(actions, packed)                the env-step alone
  step+fused:  (a)  ... then gait.step(done, reward, in place, components, body_force, feet): ONE launch
  step+read+torch: (b)  ... then sensor.read(done, ...) and the seven terms, the weights and the reward add in torch
  step+read:   (c)  ... then sensor.read(done, ...) alone (re-measured here; the parent commit's figures are profiles/r25)

Each side is timed eagerly (host clock around `reps` calls that end in a synchronise) and as a hipGraph of one call (torch.cuda.graph),
all sides in alternating rounds in this one process on the same build; the median of the rounds is reported with their spread
(max - min).  The robots stand on the floor (a settled rollout), so every foot lane runs the whole contact law.  The method is
tools/contact_sensor_rate.py's.

usage (GPU box): python tools/gait_reward_rate.py [--rounds 5] [--reps 500] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.contact import ContactSensor
from quadruped_gym_amd.gait import GaitReward
from quadruped_gym_amd.sim import BatchedSim

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=500)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
SIZES = (4096, 32768)
WEIGHTS = {"feet_air_time": 2.0, "feet_slip": -0.25, "feet_clearance": -30.0, "touchdown_speed": -0.5, "feet_contact_force": -0.01,
           "body_contact": -1.0, "flight": 0.75}
THRESHOLD, AIR, CLEAR, FMAX = 1.0, 0.02, 0.05, 20.0
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
    sensor = ContactSensor(sim, THRESHOLD)
    gait = GaitReward(sensor, WEIGHTS, air_time_target=AIR, clearance_target=CLEAR, max_contact_force=FMAX)
    actions = torch.tensor([0.0, 0.0, -0.5] * 4, device=dev).repeat(n, 1).contiguous()
    packed = torch.zeros((n, sim.obs_dim + 2), device=dev)
    force, feet = torch.empty((n, 13, 3), device=dev), torch.empty((n, 4, 12), device=dev)
    comps = torch.empty((n, 7), device=dev)
    for _ in range(150):                                     # the robots settle on their feet
        sim.step_device_packed(actions, packed)
    sensor.read(body_force=force, feet=feet)
    torch.cuda.synchronize()
    standing = float((feet[:, :, 6].sum(1) > 0).float().mean())
    reward, done = packed[:, sim.obs_dim], packed[:, sim.obs_dim + 1]
    w = torch.tensor([WEIGHTS[k] for k in GaitReward.TERMS], device=dev)
    non_feet = torch.tensor([b for b in range(13) if b not in (3, 6, 9, 12)], device=dev)
    foot_bodies = torch.tensor([3, 6, 9, 12], device=dev)

    def step():
        sim.step_device_packed(actions, packed)

    def fused():
        sim.step_device_packed(actions, packed)
        gait.step(done, reward, reward, comps, body_force=force, feet=feet)

    def read():
        sim.step_device_packed(actions, packed)
        sensor.read(done=done, body_force=force, feet=feet)

    def read_torch():
        sim.step_device_packed(actions, packed)
        sensor.read(done=done, body_force=force, feet=feet)
        c, td = feet[:, :, 6], feet[:, :, 7]
        planar = feet[:, :, 3] ** 2 + feet[:, :, 4] ** 2
        fz = force[:, :, 2]
        terms = torch.stack([(td * (feet[:, :, 10] - AIR)).sum(1), (c * planar).sum(1),
                             ((1 - c) * (feet[:, :, 2] - CLEAR) ** 2 * planar.sqrt()).sum(1), (td * feet[:, :, 5] ** 2).sum(1),
                             (fz[:, foot_bodies] - FMAX).clamp_min(0).sum(1), (fz[:, non_feet] > THRESHOLD).sum(1).float(),
                             (c.sum(1) == 0).float()], dim=1)
        torch.mul(terms * w, (done == 0).unsqueeze(1), out=comps)
        reward.add_(comps.sum(1))

    result = time_sides({"step": step, "step+fused": fused, "step+read": read, "step+read+torch": read_torch})
    for mode in ("eager", "graph"):
        s, a, c, b = (result[(mode, k)] for k in ("step", "step+fused", "step+read", "step+read+torch"))
        say(f"{n:6d} envs  {mode:5s}: step {s[0]:6.1f} (spread {s[1]:4.1f})   (a) step+fused {a[0]:6.1f} (spread {a[1]:4.1f})   "
            f"(b) step+read+torch {b[0]:6.1f} (spread {b[1]:4.1f})   (c) step+read {c[0]:6.1f} (spread {c[1]:4.1f}) us   "
            f"fused adds {a[0] - s[0]:5.1f} us, read+torch {b[0] - s[0]:6.1f} us, read alone {c[0] - s[0]:5.1f} us   "
            f"[{sim.last_step_kernel}; {100 * standing:.0f} % of the robots on their feet]")
    gait.close()
    sensor.close()
    sim.close()


say(f"# tools/gait_reward_rate.py: {args.rounds} alternated rounds of {args.reps} calls, median us per call; build "
    f"{_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
for n in SIZES:
    measure(n)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
