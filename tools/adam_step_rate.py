"""What FusedMlpPolicy.adam_step (two launches: gradient-norm clipping, Adam and both operand images) and .normalize_advantages (one
launch) cost against the torch ops they replace.  Nets: 33-64-64-12 (plain) and 260-256-256-128-12 (po_wide), actor and critic towers.

  step:       adam_step(grad)  against  clip_grad_norm_([flat], 0.5) + opt.step() + update_from(flat)  with opt = torch.optim.Adam([flat])
              as it comes (cannot be captured: its step count lives on the host), with capturable=True, and with fused=True, capturable=True
  normalise:  normalize_advantages(adv, out)  against  (adv - adv.mean()) / (adv.std() + 1e-8)  at 4096 and 65 536 rows

Each side is timed eagerly (host clock around `reps` calls that end in a synchronise) and, where it can be captured, as a hipGraph of one
call (torch.cuda.graph), all sides in alternating rounds in this one process; the median of the rounds is reported with their spread
(max - min).  The step sides start from the same parameters and gradient and are compared after three steps before timing.

usage (GPU box): python tools/adam_step_rate.py [--shapes plain po_wide] [--batch 4096 65536] [--rounds 7] [--reps 1000] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.policy import FusedMlpPolicy

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["plain", "po_wide"])
ap.add_argument("--batch", type=int, nargs="+", default=[4096, 65536])
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=1000)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
SHAPES = {"plain": (33, (64, 64), 12), "po_wide": (260, (256, 256, 128), 12)}
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def time_sides(sides, capturable):
    """``{(mode, name): (median us/call, spread)}`` of the callables ``sides``; ``capturable`` names those that also run as a graph."""
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        for fn in sides.values():
            for _ in range(3):
                fn()
    side.synchronize()
    graphs = {}
    for name in capturable:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            sides[name]()
        graphs[name] = g
    result = {}
    for mode, names in (("eager", list(sides)), ("graph", list(capturable))):
        calls = {name: (graphs[name].replay if mode == "graph" else sides[name]) for name in names}
        times = {name: [] for name in names}
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


def report(label, result, ours):
    for mode in ("eager", "graph"):
        mine = result[(mode, ours)]
        say(f"{label}  {mode:5s}: {ours} {mine[0]:8.1f} (spread {mine[1]:6.1f}) us/call")
        for (m, name), (med, spread) in result.items():
            if m == mode and name != ours:
                say(f"{label}  {mode:5s}:   {name:28s} {med:8.1f} (spread {spread:6.1f})  torch / fused {med / mine[0]:5.2f}")


def measure_step(shape):
    obs_dim, hidden, act_dim = SHAPES[shape]
    torch.manual_seed(0)
    pol = FusedMlpPolicy(obs_dim, hidden, act_dim, out_tanh=False, value=True)
    start = torch.randn(pol.n_params, device=dev) * 0.1
    grad = torch.randn(pol.n_params, device=dev) * 0.01
    pol.update_from(start)
    pol.reserve_grad(4096)                               # as in training: both operand images follow every update
    pol.reserve_adam()
    twins, flats, opts = {}, {}, {}
    for name, kw in (("Adam", {}), ("Adam capturable", dict(capturable=True)), ("Adam fused capturable", dict(fused=True, capturable=True))):
        twins[name] = FusedMlpPolicy(obs_dim, hidden, act_dim, out_tanh=False, value=True)
        twins[name].reserve_grad(4096)
        flats[name] = start.clone().requires_grad_(True)
        flats[name].grad = grad.clone()
        opts[name] = torch.optim.Adam([flats[name]], lr=3e-4, **kw)

    def torch_side(name):
        def run():
            # (clip_grad_norm_ scales the gradient in place: from the second call on its norm is 0.5 and the same ops run with coef 1)
            torch.nn.utils.clip_grad_norm_([flats[name]], 0.5)
            opts[name].step()
            twins[name].update_from(flats[name].detach())
        return run

    sides = {"adam_step": lambda: pol.adam_step(grad)}
    sides.update({name: torch_side(name) for name in twins})
    result = time_sides(sides, ["adam_step", "Adam capturable", "Adam fused capturable"])
    report(f"{shape:8s} step {pol.n_params:6d} params", result, "adam_step")
    for p in [pol] + list(twins.values()):
        p.close()


def check_step(shape):
    """Three steps of both paths from the same start: the largest difference of the parameters, in learning rates."""
    obs_dim, hidden, act_dim = SHAPES[shape]
    torch.manual_seed(1)
    pol = FusedMlpPolicy(obs_dim, hidden, act_dim, out_tanh=False, value=True)
    flat = (torch.randn(pol.n_params, device=dev) * 0.1).requires_grad_(True)
    pol.update_from(flat.detach())
    pol.reserve_adam()
    opt = torch.optim.Adam([flat], lr=3e-4)
    out = torch.empty(pol.n_params, device=dev)
    for _ in range(3):
        grad = torch.randn(pol.n_params, device=dev) * 0.01
        pol.adam_step(grad, params_out=out)
        flat.grad = grad.clone()
        torch.nn.utils.clip_grad_norm_([flat], 0.5)
        opt.step()
    torch.cuda.synchronize()
    say(f"{shape:8s} three steps, largest |adam_step - torch| over the parameters: {float((out - flat.detach()).abs().max()) / 3e-4:.2e} learning rates")
    pol.close()


def measure_normalise(B):
    pol = FusedMlpPolicy(33, (64, 64), 12)
    torch.manual_seed(2)
    adv, out = torch.randn(B, device=dev) * 3 + 0.7, torch.empty(B, device=dev)
    keep = {}

    def torch_side():
        keep["out"] = (adv - adv.mean()) / (adv.std() + 1e-8)

    sides = {"normalize_advantages": lambda: pol.normalize_advantages(adv, out=out), "torch expression": torch_side}
    result = time_sides(sides, list(sides))
    torch.cuda.synchronize()
    say(f"normalise B {B:6d}  largest |fused - torch|: {float((out - keep['out']).abs().max()):.2e}")
    report(f"normalise B {B:6d}", result, "normalize_advantages")
    pol.close()


say(f"# tools/adam_step_rate.py: {args.rounds} alternated rounds of {args.reps} calls, median us/call; build "
    f"{_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
for shape in args.shapes:
    check_step(shape)
    measure_step(shape)
for B in args.batch:
    measure_normalise(B)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
