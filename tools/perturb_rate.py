"""What the perturbation layer's two launches per env-step (Perturbation.perturb_actions + .observe: csrc/qg_perturb.hip) cost against
the torch expression that comes closest, at 4096 x 33 (the plain pack), 4096 x 260 and 32 768 x 260 (ten partially observable frames).

  perturb:  perturb_actions(actions, out) ; observe(obs, done)          delays (0, 3) env-steps, action noise, noise and bias on the
                                                                        sensor columns (9 of 33; 11 of 26 per frame)
  torch:    ring[slot] = actions ; v = ring.view(-1, 12).index_select(0, rows) ; out = v + action_std * randn_like(v)
            obs += randn_like(obs) * std_row + bias                     std_row zero on the quiet columns, bias [n, D] drawn once

The torch side is cheaper in what it does, not only in how: its noise is not keyed by env and episode, a stacked frame gets a new value
in every slot, `slot` and `rows` stand still (a real ring needs two more index kernels per step), no episode ever ends.  It is the floor of
what a user would write, so the ratio below is a lower bound on what the layer saves -- or an upper bound on what it costs.

Each side is timed eagerly (host clock around `reps` calls that end in a synchronise) and as a hipGraph of one call (torch.cuda.graph),
all sides in alternating rounds in this one process; the median of the rounds is reported with their spread (max - min).

usage (GPU box): python tools/perturb_rate.py [--rounds 7] [--reps 1000] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.perturb import Perturbation, column_stds

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=1000)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
SHAPES = ((4096, 1, 33), (4096, 10, 26), (32768, 10, 26))          # (n, window, frame_dim)
SENSORS = {33: {"accel": 0.01, "gyro": 0.01, "body_vel": 0.01}, 26: {"gyro": 0.01, "accel": 0.01, "euler": 0.005, "body_vel": 0.01}}
DELAYS, ACTION_STD = (0, 3), 0.02
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


def measure(n, window, frame):
    D, M = window * frame, DELAYS[1] + 1
    torch.manual_seed(0)
    pz = Perturbation(n, frame, window, obs_std=SENSORS[frame], bias_std=SENSORS[frame], action_std=ACTION_STD, delays=DELAYS, done_row="reset",
                      seed=1)
    actions, delayed = torch.rand((n, 12), device=dev) * 2 - 1, torch.empty((n, 12), device=dev)
    obs, done = torch.randn((n, D), device=dev), torch.zeros(n, device=dev, dtype=torch.uint8)
    done[::97] = 1                                       # about one env in a hundred finishes at every call

    def ours():
        pz.perturb_actions(actions, out=delayed)
        pz.observe(obs, done)

    std_row = torch.from_numpy(column_stds(SENSORS[frame], frame)).repeat(window).to(dev)
    bias = torch.randn((n, D), device=dev) * std_row
    ring = torch.zeros((M, n, 12), device=dev)
    rows = (torch.randint(0, M, (n,), device=dev) * n + torch.arange(n, device=dev))
    t_obs, t_out = torch.randn((n, D), device=dev), torch.empty((n, 12), device=dev)

    def torch_side():
        ring[1] = actions
        v = ring.view(-1, 12).index_select(0, rows)
        torch.add(v, torch.randn_like(v), alpha=ACTION_STD, out=t_out)
        t_obs.add_(torch.randn_like(t_obs) * std_row + bias)

    result = time_sides({"perturb": ours, "torch": torch_side})
    for mode in ("eager", "graph"):
        mine, theirs = result[(mode, "perturb")], result[(mode, "torch")]
        say(f"{n:6d} x {D:3d}  {mode:5s}: perturb {mine[0]:7.1f} (spread {mine[1]:5.1f})   torch {theirs[0]:7.1f} (spread {theirs[1]:5.1f}) us per "
            f"env-step   torch / perturb {theirs[0] / mine[0]:5.2f}")
    pz.close()


say(f"# tools/perturb_rate.py: {args.rounds} alternated rounds of {args.reps} calls, median us per env-step (two launches); build "
    f"{_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
for shape in SHAPES:
    measure(*shape)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
