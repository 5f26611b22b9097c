"""What the fused policy launch (quadruped_gym_amd.policy.FusedMlpPolicy) costs against the same policy as torch modules, alone and in
the closed loop with the env step.  Shapes: 33-64-64-12 on the plain step's packed rows, 260-64-64-12 and 260-256-256-128-12 (the
reference's net_arch, src/train_quadruped.py:52-55) on the partially observed walking step; each as the bare actor and as what a PPO
rollout collects (sampled action, log-probability, critic value).  Every configuration is a hipGraph of 8 closed-loop steps on one
stream (capture and timing as tools/closed_loop_demo.py); the torch and the fused graphs are timed in alternating rounds in this one
process, the median of the rounds is reported with their spread (max - min).

usage (GPU box): python tools/policy_rate.py [--envs 4096 32768] [--rounds 7] [--steps 800] [--waves-ab] [--out FILE]
--waves-ab adds the fused policy pinned to one and to four waves per 16-env tile (QG_POLICY_WAVES), the A/B behind the launch heuristic."""
import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
from quadruped_gym_amd.policy import FusedMlpPolicy
from quadruped_gym_amd.sim import BatchedSim

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="+", default=[4096, 32768])
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=800)
ap.add_argument("--waves-ab", action="store_true")
ap.add_argument("--shapes", nargs="+", default=["plain", "po", "po_wide"])
ap.add_argument("--out", default=None)
args = ap.parse_args()

G = 8
dev = torch.device("cuda:0")
SHAPES = {"plain": (33, (64, 64), 12), "po": (260, (64, 64), 12), "po_wide": (260, (256, 256, 128), 12)}
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def tower(obs_dim, hidden, out_dim, out_tanh):
    dims, mods = (obs_dim,) + tuple(hidden), []
    for i in range(len(hidden)):
        mods += [torch.nn.Linear(dims[i], dims[i + 1]), torch.nn.Tanh()]
    mods.append(torch.nn.Linear(dims[-1], out_dim))
    if out_tanh:
        mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods).to(dev)


def fused_policy(shape, full, actor, critic, log_std, waves=None):
    obs_dim, hidden, act_dim = SHAPES[shape]
    if waves:
        os.environ["QG_POLICY_WAVES"] = str(waves)          # read once, by qg_policy_create
    pol = FusedMlpPolicy(obs_dim, hidden, act_dim, out_tanh=True, value=full)
    os.environ.pop("QG_POLICY_WAVES", None)
    pol.load_module(actor, critic if full else None, log_std)
    return pol


def measure(n, shape, full, plain_sim, po_env):
    obs_dim, hidden, act_dim = SHAPES[shape]
    torch.manual_seed(0)
    actor = tower(obs_dim, hidden, act_dim, True)
    critic = tower(obs_dim, hidden, 1, False)
    log_std = torch.full((act_dim,), -0.5, device=dev)
    std = log_std.exp()
    acts = torch.zeros((n, act_dim), device=dev)
    lp, val = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    eps = torch.randn((G, n, act_dim), device=dev)
    rew, done = torch.zeros(n, device=dev), torch.zeros(n, device=dev, dtype=torch.uint8)
    if shape == "plain":
        rows = torch.zeros((n, 35), device=dev)
        obs = rows[:, :33]                                   # the policy reads the packed rows in place

        def env_step():
            plain_sim.step_device_packed(acts, rows)
    else:
        obs = torch.from_numpy(po_env.reset()).to(dev)

        def env_step():
            po_env.step_tensor(acts, obs, rew, done)         # obs is overwritten in place with the next stack

    def torch_policy(k):
        with torch.no_grad():
            mean = actor(obs)
            if full:
                acts.copy_(mean + std * eps[k])
                lp.copy_((-0.5 * eps[k] * eps[k] - log_std - HALF_LOG_2PI).sum(-1))
                val.copy_(critic(obs)[:, 0])
            else:
                acts.copy_(mean)

    variants = {"torch": torch_policy}
    pols = {"fused": fused_policy(shape, full, actor, critic, log_std)}
    if args.waves_ab:
        pols["fused_w1"] = fused_policy(shape, full, actor, critic, log_std, 1)
        pols["fused_w4"] = fused_policy(shape, full, actor, critic, log_std, 4)
    for name, pol in pols.items():
        if full:
            variants[name] = lambda k, pol=pol: pol.forward(obs, acts, eps=eps[k], log_prob=lp, value=val)
        else:
            variants[name] = lambda k, pol=pol: pol.forward(obs, acts)

    side = torch.cuda.Stream(dev)
    result = {}
    for with_env in (False, True):
        graphs = {}
        for name, fn in variants.items():
            def loop():
                for k in range(G):
                    fn(k)
                    if with_env:
                        env_step()
            with torch.cuda.stream(side):
                loop()
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                loop()
            graphs[name] = g
        times = {name: [] for name in graphs}
        reps = max(1, args.steps // G)
        with torch.cuda.stream(side):
            for name, g in graphs.items():
                for _ in range(10):
                    g.replay()
            side.synchronize()
            for _ in range(args.rounds):
                for name, g in graphs.items():          # alternated: one round of each in turn
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        g.replay()
                    side.synchronize()
                    times[name].append((time.perf_counter() - t0) / (reps * G) * 1e6)
        ok = bool(torch.isfinite(acts).all())
        for name, ts in times.items():
            result[(name, with_env)] = (statistics.median(ts), min(ts), max(ts))
        what = "policy + env step" if with_env else "policy alone     "
        text = "  ".join(f"{name} {statistics.median(ts):7.2f} (spread {max(ts) - min(ts):5.2f})" for name, ts in times.items())
        say(f"{n:6d} envs  {shape:8s} {'actor+critic+logp' if full else 'actor only       '}  {what}: {text}  us/step  finite {ok}")
        del graphs
    t, f = result[("torch", False)], result[("fused", False)]
    spread = max(t[2] - t[1], f[2] - f[1])
    say(f"{n:6d} envs  {shape:8s} {'actor+critic+logp' if full else 'actor only       '}  fused below torch by {t[0] - f[0]:6.2f} us "
        f"(largest spread between rounds {spread:5.2f} us): {'yes' if t[0] - f[0] > spread else 'NO'}; closed loop {result[('torch', True)][0]:6.2f} -> "
        f"{result[('fused', True)][0]:6.2f} us/step")
    for pol in pols.values():
        pol.close()


def task():
    t = _abi.default_task()
    t.auto_reset, t.use_fall, t.fall_height = 1, 1, 0.05
    return t


say(f"# tools/policy_rate.py: hipGraph of {G} closed-loop steps, {args.rounds} alternated rounds of {args.steps} steps, median us/step; "
    f"build {_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
for n in args.envs:
    plain_sim = po_env = None
    if "plain" in args.shapes:
        plain_sim = BatchedSim(n, task=task())
        plain_sim.reset(seed=0)
    if any(s != "plain" for s in args.shapes):
        po_env = POWalkingQuadrupedVecEnv(n, obs_window=10, random_controls=True, random_init=True, device_commands=True,
                                          reset_options={"min_speed": 0.0, "max_speed": 0.5}, settling_time=0.5, max_time=10.0)
    for shape in args.shapes:
        for full in (False, True):
            measure(n, shape, full, plain_sim, po_env)
    if plain_sim:
        plain_sim.close()
    if po_env:
        po_env.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
