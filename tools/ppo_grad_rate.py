"""What FusedMlpPolicy.ppo_grad (three launches: loss, statistics and the flat gradient of one PPO minibatch) costs against the path it
replaces: the same policy as torch float32 modules, their forward pass, SB3's loss, backward() and the concatenation of the .grads into
one flat vector.  Nets: 33-64-64-12 (plain) and 260-256-256-128-12 (po_wide), actor and critic towers; minibatches of 4096 and 65 536
rows.  Each side is timed eagerly (host clock around `reps` calls that end in a synchronise) and as a hipGraph of one call
(torch.cuda.graph), the two sides in alternating rounds in this one process; the median of the rounds is reported with their spread
(max - min).  Both sides are checked against each other on the timed inputs before timing.

usage (GPU box): python tools/ppo_grad_rate.py [--batch 4096 65536] [--shapes plain po_wide] [--rounds 7] [--reps 50] [--out FILE]"""
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
ap.add_argument("--batch", type=int, nargs="+", default=[4096, 65536])
ap.add_argument("--shapes", nargs="+", default=["plain", "po_wide"])
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
SHAPES = {"plain": (33, (64, 64), 12), "po_wide": (260, (256, 256, 128), 12)}
CLIP, CLIP_VF, ENT, VF = 0.2, 0.3, 0.01, 0.5
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


def measure(shape, B):
    obs_dim, hidden, act_dim = SHAPES[shape]
    torch.manual_seed(0)
    actor, critic = tower(obs_dim, hidden, act_dim), tower(obs_dim, hidden, 1)
    log_std = torch.nn.Parameter(torch.full((act_dim,), -1.2, device=dev))
    params = list(actor.parameters()) + [log_std] + list(critic.parameters())        # the canonical order
    pol = FusedMlpPolicy(obs_dim, hidden, act_dim, out_tanh=False, value=True)
    pol.load_module(actor, critic, log_std)
    pol.reserve_grad(B)
    with torch.no_grad():
        obs = torch.randn((B, obs_dim), device=dev)
        acts = actor(obs) + log_std.exp() * torch.randn((B, act_dim), device=dev)
        logp = torch.distributions.Normal(actor(obs), log_std.exp()).log_prob(acts).sum(1)
        batch = Samples(obs, acts, critic(obs)[:, 0] + 0.3 * torch.randn(B, device=dev), logp + 0.3 * torch.randn(B, device=dev),
                        torch.randn(B, device=dev), torch.randn(B, device=dev))
    flat_t, flat_f, stats = torch.zeros(pol.n_params, device=dev), torch.zeros(pol.n_params, device=dev), torch.zeros(8, device=dev)

    def torch_side():
        for p in params:
            p.grad = None
        dist = torch.distributions.Normal(actor(batch.observations), torch.ones_like(log_std) * log_std.exp(), validate_args=False)   # (validation synchronises: not in a capture)
        log_prob = dist.log_prob(batch.actions).sum(dim=1)
        ratio = torch.exp(log_prob - batch.old_log_prob)
        policy_loss = -torch.min(batch.advantages * ratio, batch.advantages * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean()
        values = critic(batch.observations).flatten()
        values = batch.old_values + torch.clamp(values - batch.old_values, -CLIP_VF, CLIP_VF)
        value_loss = torch.nn.functional.mse_loss(batch.returns, values)
        loss = policy_loss + ENT * -torch.mean(dist.entropy().sum(dim=1)) + VF * value_loss
        loss.backward()
        torch.cat([p.grad.reshape(-1) for p in params], out=flat_t)

    def fused_side():
        pol.ppo_grad(batch, flat_f, stats, clip_range=CLIP, clip_range_vf=CLIP_VF, ent_coef=ENT, vf_coef=VF)

    sides = {"torch": torch_side, "fused": fused_side}
    side = torch.cuda.Stream(dev)
    graphs = {}
    with torch.cuda.stream(side):
        for fn in sides.values():
            for _ in range(3):
                fn()
    side.synchronize()
    worst = float((flat_t - flat_f).abs().max() / flat_t.abs().max())
    for name, fn in sides.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn()
        graphs[name] = g
    result = {}
    for mode in ("eager", "graph"):
        times = {name: [] for name in sides}
        with torch.cuda.stream(side):
            for name in sides:
                for _ in range(5):
                    graphs[name].replay() if mode == "graph" else sides[name]()
            side.synchronize()
            for _ in range(args.rounds):
                for name in sides:                       # alternated: one round of each in turn
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        graphs[name].replay() if mode == "graph" else sides[name]()
                    side.synchronize()
                    times[name].append((time.perf_counter() - t0) / args.reps * 1e6)
        for name, ts in times.items():
            result[(mode, name)] = (statistics.median(ts), max(ts) - min(ts))
    for mode in ("eager", "graph"):
        t, f = result[(mode, "torch")], result[(mode, "fused")]
        say(f"{shape:8s} B {B:6d}  {mode:5s}: torch {t[0]:9.1f} (spread {t[1]:7.1f})  fused {f[0]:9.1f} (spread {f[1]:7.1f})  us/call  "
            f"torch / fused {t[0] / f[0]:5.2f}")
    say(f"{shape:8s} B {B:6d}  largest |fused - torch| over the flat gradient, relative to its largest element: {worst:.2e}")
    del graphs
    pol.close()


say(f"# tools/ppo_grad_rate.py: one PPO minibatch (loss + flat gradient), {args.rounds} alternated rounds of {args.reps} calls, median "
    f"us/call; build {_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
for shape in args.shapes:
    for B in args.batch:
        measure(shape, B)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
