"""What FusedMlpPolicy.distill_grad (three launches: the imitation loss, its statistics and the flat gradient of one minibatch) costs
against the path it replaces: the same student as torch float32 modules, their forward pass, the same loss, backward() and the
concatenation of the .grads into one flat vector.  Nets: 33-64-64-12 (plain) and 260-256-256-128-12 (po_wide), with a critic tower
(whose entries the loss does not reach: zeros on both sides); minibatches of 4096 and 65 536 rows; MSE and KL mode, per-row weights on.
Each side is timed eagerly (host clock around `reps` calls that end in a synchronise) and as a hipGraph of one call, the two sides in
alternating rounds in this one process; the median of the rounds is reported with their spread (max - min).  Both sides are checked
against each other on the timed inputs before timing.

--neighbours times what the pass shares a handle with instead -- `ppo_grad` and `forward` (with log-prob and value) of the same nets
and sizes, no torch side -- for an A/B of two builds of the library: run it once per build with QUADGYM_LIB set, alternating the
builds.  It also runs on a build from before the pass existed.

usage (GPU box): python tools/distill_rate.py [--neighbours] [--batch 4096 65536] [--shapes plain po_wide] [--rounds 7] [--reps 50] [--out FILE]"""
import argparse
import collections
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi

ap = argparse.ArgumentParser()
ap.add_argument("--neighbours", action="store_true")
ap.add_argument("--batch", type=int, nargs="+", default=[4096, 65536])
ap.add_argument("--shapes", nargs="+", default=["plain", "po_wide"])
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=None)
args = ap.parse_args()

if args.neighbours and not hasattr(ctypes.CDLL(_abi.library_path()), "qg_policy_distill_grad_device"):
    del _abi.PROTOTYPES["qg_policy_distill_grad_device"]          # an older build: everything --neighbours calls is there
from quadruped_gym_amd.policy import FusedMlpPolicy  # noqa: E402

dev = torch.device("cuda:0")
SHAPES = {"plain": (33, (64, 64), 12), "po_wide": (260, (256, 256, 128), 12)}
COEF = 0.5
Samples = collections.namedtuple("Samples", ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns"])
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def tower(obs_dim, hidden, out_dim):
    dims, mods = (obs_dim,) + tuple(hidden), []
    for i in range(len(hidden)):
        mods += [torch.nn.Linear(dims[i], dims[i + 1]), torch.nn.Tanh()]
    mods.append(torch.nn.Linear(dims[-1], out_dim))
    return torch.nn.Sequential(*mods).to(dev)


def time_sides(sides):
    """``{(mode, name): (median us per call, spread)}`` of the callables, eagerly and as hipGraphs, in alternated rounds."""
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
                for _ in range(5):
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


def build(shape, B):
    obs_dim, hidden, act_dim = SHAPES[shape]
    torch.manual_seed(0)
    actor, critic = tower(obs_dim, hidden, act_dim), tower(obs_dim, hidden, 1)
    log_std = torch.nn.Parameter(torch.full((act_dim,), -1.2, device=dev))
    pol = FusedMlpPolicy(obs_dim, hidden, act_dim, out_tanh=False, value=True)
    pol.load_module(actor, critic, log_std)
    pol.reserve_grad(B)
    return actor, critic, log_std, pol


def measure(shape, B):
    obs_dim, hidden, act_dim = SHAPES[shape]
    actor, critic, log_std, pol = build(shape, B)
    params = list(actor.parameters()) + [log_std] + list(critic.parameters())        # the canonical order
    teacher = tower(obs_dim, hidden, act_dim)
    with torch.no_grad():
        obs = torch.randn((B, obs_dim), device=dev)
        target = teacher(obs).contiguous()
        target_log_std = torch.full((act_dim,), -1.0, device=dev)
        weights = torch.rand(B, device=dev) + 0.5
    flat_t, flat_f, stats = torch.zeros(pol.n_params, device=dev), torch.zeros(pol.n_params, device=dev), torch.zeros(8, device=dev)
    for mode in ("mse", "kl"):
        def torch_side():
            for p in params:
                p.grad = None
            diff = actor(obs) - target
            if mode == "mse":
                rows = (diff ** 2).sum(dim=1)
            else:
                rows = (log_std - target_log_std + (torch.exp(2 * target_log_std) + diff ** 2) / (2 * torch.exp(2 * log_std)) - 0.5).sum(dim=1)
            (COEF * (rows * weights).sum() / B).backward()
            torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params], out=flat_t)

        def fused_side():
            pol.distill_grad(obs, target, flat_f, stats, loss=mode, coef=COEF, target_log_std=target_log_std if mode == "kl" else None,
                             weights=weights)

        torch_side(), fused_side()
        torch.cuda.synchronize()
        worst = float((flat_t - flat_f).abs().max() / flat_t.abs().max())
        result = time_sides({"torch": torch_side, "fused": fused_side})
        for how in ("eager", "graph"):
            t, f = result[(how, "torch")], result[(how, "fused")]
            say(f"{shape:8s} B {B:6d} {mode:3s} {how:5s}: torch {t[0]:9.1f} (spread {t[1]:7.1f})  fused {f[0]:9.1f} (spread {f[1]:7.1f})  us/call  "
                f"torch / fused {t[0] / f[0]:5.2f}")
        say(f"{shape:8s} B {B:6d} {mode:3s} largest |fused - torch| over the flat gradient, relative to its largest element: {worst:.2e}")
    pol.close()


def neighbours(shape, B):
    obs_dim, hidden, act_dim = SHAPES[shape]
    actor, critic, log_std, pol = build(shape, B)
    with torch.no_grad():
        obs = torch.randn((B, obs_dim), device=dev)
        acts = actor(obs) + log_std.exp() * torch.randn((B, act_dim), device=dev)
        logp = torch.distributions.Normal(actor(obs), log_std.exp()).log_prob(acts).sum(1)
        batch = Samples(obs, acts, critic(obs)[:, 0] + 0.3 * torch.randn(B, device=dev), logp + 0.3 * torch.randn(B, device=dev),
                        torch.randn(B, device=dev), torch.randn(B, device=dev))
    grad, stats = torch.zeros(pol.n_params, device=dev), torch.zeros(8, device=dev)
    eps, out, lp, val = torch.randn((B, act_dim), device=dev), torch.zeros((B, act_dim), device=dev), torch.zeros(B, device=dev), torch.zeros(B, device=dev)
    result = time_sides({"ppo_grad": lambda: pol.ppo_grad(batch, grad, stats, clip_range=0.2, clip_range_vf=0.3, ent_coef=0.01, vf_coef=0.5),
                         "forward": lambda: pol.forward(obs, out, eps=eps, log_prob=lp, value=val)})
    for how in ("eager", "graph"):
        g, f = result[(how, "ppo_grad")], result[(how, "forward")]
        say(f"{shape:8s} B {B:6d} {how:5s}: ppo_grad {g[0]:9.1f} (spread {g[1]:6.1f})  forward {f[0]:8.1f} (spread {f[1]:6.1f})  us/call")
    pol.close()


what = "ppo_grad and forward (--neighbours)" if args.neighbours else "one distillation minibatch (loss + flat gradient)"
say(f"# tools/distill_rate.py: {what}, {args.rounds} alternated rounds of {args.reps} calls, median us/call; build "
    f"{_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
for shape in args.shapes:
    for B in args.batch:
        (neighbours if args.neighbours else measure)(shape, B)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
