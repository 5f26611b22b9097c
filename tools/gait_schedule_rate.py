"""What the commanded gait schedule costs behind the env-step at 4096 and 32 768 envs, around the walking env (33 observation
columns) and the partially observable env at obs_window = 10 (260 columns): the fused launch (csrc/qg_sched.hip) against
sensor.read(advance=False) -- the floor: the same forces and foot kinematics -- and against that read followed by the closest torch
expression of the phase advance, the ten clock columns, the four terms and the reward add.

  step:                 env.step_tensor(actions, obs, reward, done)            the env-step alone
  step+fused:      (a)  ... then schedule.step(done, reward, in place, components, obs=obs, out=wide): ONE launch
  step+read+torch: (b)  ... then sensor.read(advance=False) and phase, columns, terms, weights, reward add and the row copy in torch
                        (the torch side keeps one gait and frequency per env: it leaves out the per-episode redraw, which has no short
                        torch expression -- in its favour)
  step+read:       (c)  ... then sensor.read(advance=False) alone

Each side is timed eagerly (host clock around `reps` calls that end in a synchronise) and as a hipGraph of one call (torch.cuda.graph),
all sides in alternating rounds in this one process on the same build; the median of the rounds is reported with their spread
(max - min).  The method is tools/gait_reward_rate.py's.

usage (GPU box): python tools/gait_schedule_rate.py [--rounds 5] [--reps 500] [--out FILE]"""
import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv, WalkingQuadrupedVecEnv
from quadruped_gym_amd.schedule import GAITS, GaitSchedule

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=500)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
SIZES = (4096, 32768)
TABLE = ("trot", "pace", "bound", "pronk", "walk")
WEIGHTS = {"swing_force": -0.5, "stance_velocity": -0.25, "swing_height": -30.0, "contact_match": 0.125}
THRESHOLD, KAPPA, SIGMA_F, SIGMA_V, HEIGHT, FREQ = 1.0, 1.0 / 256, 5.0, 0.5, 0.05, (1.0, 3.0)
WALK = dict(device_commands=True, random_controls=True, nan_direction=False)
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


def measure(kind, n):
    env = WalkingQuadrupedVecEnv(n, **WALK) if kind == "walking" else POWalkingQuadrupedVecEnv(n, obs_window=10, **WALK)
    env.reset()
    O = env.obs_dim
    sensor = env.contact_sensor(THRESHOLD)
    sched = GaitSchedule(sensor, TABLE, FREQ, WEIGHTS, random_phase=True, done_row="reset" if kind == "po" else "terminal", kappa=KAPPA,
                         sigma_force=SIGMA_F, sigma_velocity=SIGMA_V, swing_height_target=HEIGHT)
    actions = torch.tensor([0.0, 0.0, -0.5] * 4, device=dev).repeat(n, 1).contiguous()
    obs, reward, done = torch.zeros((n, O), device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev, dtype=torch.uint8)
    wide, comps = torch.zeros((n, O + 10), device=dev), torch.zeros((n, 4), device=dev)
    force, feet = torch.empty((n, 13, 3), device=dev), torch.empty((n, 4, 12), device=dev)
    for _ in range(150):                                     # the robots settle on their feet
        env.step_tensor(actions, obs, reward, done)
    # the torch side's tables: one gait and frequency per env, the integers in int64
    drawn = sched.gaits()
    off = torch.tensor([[int(round(o * 2 ** 32)) % 2 ** 32 for o in GAITS[name][0]] for name in TABLE], device=dev)[torch.from_numpy(drawn["gait"]).to(dev).long()]
    D = torch.tensor([int(round(GAITS[name][1] * 2 ** 32)) for name in TABLE], device=dev)[torch.from_numpy(drawn["gait"]).to(dev).long()]
    freq = torch.from_numpy(drawn["freq"]).to(dev)
    dt = float(env.model.opt.timestep) * env.frame_skip
    dphi = torch.round(freq.double() * dt * 2 ** 32).long()
    phi = torch.from_numpy(drawn["phi"].astype("int64")).to(dev)
    d = ((D >> 8).float() * 2.0 ** -24).unsqueeze(1)
    w = torch.tensor([WEIGHTS[k] for k in GaitSchedule.TERMS], device=dev)
    foot_bodies = torch.tensor([3, 6, 9, 12], device=dev)
    inv2k, inv_sf2, inv_sv2, mask32 = 1.0 / (2 * KAPPA), 1.0 / SIGMA_F ** 2, 1.0 / SIGMA_V ** 2, 2 ** 32 - 1

    def step():
        env.step_tensor(actions, obs, reward, done)

    def fused():
        env.step_tensor(actions, obs, reward, done)
        sched.step(done, reward, reward, comps, obs=obs, out=wide)

    def read():
        env.step_tensor(actions, obs, reward, done)
        sensor.read(advance=False, body_force=force, feet=feet)

    def read_torch():
        env.step_tensor(actions, obs, reward, done)
        sensor.read(advance=False, body_force=force, feet=feet)
        phi.add_(dphi).bitwise_and_(mask32)
        q = (phi.unsqueeze(1) + off) & mask32
        hard = q < D.unsqueeze(1)
        p = (q >> 8).float() * 2.0 ** -24
        m = torch.where(hard, torch.minimum(p, d - p), -torch.minimum(p - d, 1 - p))
        s = (0.5 + m * inv2k).clamp(0, 1)
        F, v = force[:, foot_bodies], feet[:, :, 3:6]
        terms = torch.stack([((1 - s) * (1 - torch.exp(-(F * F).sum(2) * inv_sf2))).sum(1), (s * (1 - torch.exp(-(v * v).sum(2) * inv_sv2))).sum(1),
                             ((1 - s) * (feet[:, :, 2] - HEIGHT) ** 2).sum(1), ((feet[:, :, 6] > 0.5) == hard).sum(1).float()], dim=1)
        torch.mul(terms * w, (done == 0).unsqueeze(1), out=comps)
        reward.add_(comps.sum(1))
        wide[:, :O] = obs
        wide[:, O:O + 4], wide[:, O + 4:O + 8] = torch.sin(2 * math.pi * p), torch.cos(2 * math.pi * p)
        wide[:, O + 8], wide[:, O + 9] = freq, d[:, 0]

    result = time_sides({"step": step, "step+fused": fused, "step+read": read, "step+read+torch": read_torch})
    for mode in ("eager", "graph"):
        s, a, c, b = (result[(mode, k)] for k in ("step", "step+fused", "step+read", "step+read+torch"))
        say(f"{kind:7s} {O:3d} cols {n:6d} envs  {mode:5s}: step {s[0]:6.1f} (spread {s[1]:4.1f})   (a) step+fused {a[0]:6.1f} (spread {a[1]:4.1f})   "
            f"(b) step+read+torch {b[0]:6.1f} (spread {b[1]:4.1f})   (c) step+read {c[0]:6.1f} (spread {c[1]:4.1f}) us   "
            f"fused adds {a[0] - s[0]:5.1f} us, read+torch {b[0] - s[0]:6.1f} us, read alone {c[0] - s[0]:5.1f} us")
    sched.close()
    env.close()


say(f"# tools/gait_schedule_rate.py: {args.rounds} alternated rounds of {args.reps} calls, median us per call; build "
    f"{_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
for kind in ("walking", "po"):
    for n in SIZES:
        measure(kind, n)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
