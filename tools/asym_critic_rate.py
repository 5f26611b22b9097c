"""What the critic window of FusedMlpPolicy costs: `forward` with a value buffer and `ppo_grad` of an asymmetric handle whose critic
reads the whole joint row, window (0, O + 85), against the symmetric handle (both towers on the actor's O columns) on the SAME wide rows
[n, O + 85].  Nets O-64-64-12 for O = 33 and 260; 4096 rows.  The asymmetric critic's first layer is 85 columns wider, which is the
work that is added; nothing else differs.  Each side is timed eagerly and as a hipGraph of one call, the sides in alternating rounds in
this one process; the median of the rounds is reported with their spread (max - min).

usage (GPU box): python tools/asym_critic_rate.py [--rows 4096] [--rounds 7] [--reps 200] [--out FILE]"""
import argparse
import collections
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.policy import FusedMlpPolicy

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
Samples = collections.namedtuple("Samples", ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns"])
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def time_sides(sides):
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


def measure(O):
    n, act = args.rows, 12
    torch.manual_seed(0)
    rows = torch.randn((n, O + 85), device=dev)
    pols = {"symmetric": FusedMlpPolicy(O, (64, 64), act), "asymmetric": FusedMlpPolicy(O, (64, 64), act, critic_obs=(0, O + 85))}
    for p in pols.values():
        p.update_from(0.05 * torch.randn(p.n_params, device=dev))
        p.reserve_grad(n)
    torch.cuda.synchronize()
    eps = torch.randn((n, act), device=dev)
    out = {k: (torch.zeros((n, act), device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(p.n_params, device=dev),
               torch.zeros(8, device=dev)) for k, p in pols.items()}
    batch = Samples(rows[:, :O], torch.randn((n, act), device=dev), torch.randn(n, device=dev), torch.randn(n, device=dev) - 12.0,
                    torch.randn(n, device=dev), torch.randn(n, device=dev))
    sides = {}
    for k, p in pols.items():
        a, l, v, g, s = out[k]
        sides[f"forward {k}"] = lambda p=p, a=a, l=l, v=v: p.forward(rows[:, :O], a, eps=eps, log_prob=l, value=v)
        sides[f"ppo_grad {k}"] = lambda p=p, g=g, s=s: p.ppo_grad(batch, g, s, clip_range_vf=0.3, ent_coef=0.01)
    result = time_sides(sides)
    for mode in ("eager", "graph"):
        for what in ("forward", "ppo_grad"):
            s, a = result[(mode, f"{what} symmetric")], result[(mode, f"{what} asymmetric")]
            say(f"{n} rows, {O}-64-64-12, window (0, {O + 85})  {mode:5s} {what:8s}: symmetric {s[0]:7.1f} (spread {s[1]:4.1f})   asymmetric {a[0]:7.1f} "
                f"(spread {a[1]:4.1f}) us   the wider critic adds {a[0] - s[0]:5.1f} us = {100.0 * (a[0] - s[0]) / s[0]:4.0f} %")
    for p in pols.values():
        p.close()


say(f"# tools/asym_critic_rate.py: {args.rounds} alternated rounds of {args.reps} calls, median us per call; build "
    f"{_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
for O in (33, 260):
    measure(O)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
