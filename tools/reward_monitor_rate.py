"""What one record of the reward monitor (quadruped_gym_amd.monitor.RewardMonitor, two launches) costs against the closest torch
expression under the same conditions -- float64 column means and the reward's mean / std(unbiased=False) into a ring row at a cursor
kept on the device, an `acc +=`, and the masked fold -- at 4096 x 3, 4096 x 11 and 32 768 x 11, eagerly and as a hipGraph of 8
records on one stream; and what it adds to the closed-loop step of INTEGRATION.md section 13 on the walking env (fused policy, env step
with components, running normaliser, rollout record) at 4096 envs.  The variants are timed in alternating rounds in this one process;
the median of the rounds is reported with their spread (max - min).

usage (GPU box): python tools/reward_monitor_rate.py [--rounds 7] [--steps 800] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.envs.walking import WalkingQuadrupedVecEnv
from quadruped_gym_amd.monitor import RewardMonitor
from quadruped_gym_amd.normalize import RunningNormalizer
from quadruped_gym_amd.policy import FusedMlpPolicy
from quadruped_gym_amd.rollout import DeviceRolloutBuffer

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=800)
ap.add_argument("--shapes", nargs="+", default=["4096x3", "4096x11", "32768x11"])
ap.add_argument("--loop-envs", type=int, default=4096)
ap.add_argument("--out", default=None)
args = ap.parse_args()

G = 8
CAPACITY = 4096
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


class TorchMonitor:
    """The same record in torch: everything in device tensors, the cursor included, so that a captured graph replays."""

    def __init__(self, n, C, capacity):
        f64, i64 = dict(device=dev, dtype=torch.float64), dict(device=dev, dtype=torch.int64)
        self.capacity = capacity
        self.log = torch.zeros((capacity, C + 3), **f64)
        self.acc, self.len = torch.zeros((n, C + 1), **f64), torch.zeros(n, **i64)
        self.totals = torch.zeros(C + 1, **f64)
        self.episodes, self.length_sum, self.records = torch.zeros((), **i64), torch.zeros((), **i64), torch.zeros(1, **i64)

    def record(self, comps, reward, done):
        x = torch.cat([comps, reward[:, None]], dim=1).double()
        fin = done != 0
        row = torch.cat([x.mean(0), x[:, -1].std(unbiased=False)[None], fin.sum()[None].double()])
        self.log.index_copy_(0, self.records % self.capacity, row[None])
        self.acc += x
        self.len += 1
        self.totals += (self.acc * fin[:, None]).sum(0)
        self.length_sum += (self.len * fin).sum()
        self.episodes += fin.sum()
        self.acc.masked_fill_(fin[:, None], 0.0)
        self.len.masked_fill_(fin, 0)
        self.records += 1


def timed(fn_by_name, graph):
    """Alternating rounds; returns {name: [us per step per round]}."""
    side = torch.cuda.Stream(dev)
    runs = {}
    for name, fn in fn_by_name.items():
        def loop(fn=fn):
            for _ in range(G):
                fn()
        with torch.cuda.stream(side):
            loop()
        side.synchronize()
        if graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                loop()
            runs[name] = g.replay
        else:
            runs[name] = loop
    times = {name: [] for name in runs}
    reps = max(1, args.steps // G)
    with torch.cuda.stream(side):
        for run in runs.values():
            for _ in range(10):
                run()
        side.synchronize()
        for _ in range(args.rounds):
            for name, run in runs.items():
                t0 = time.perf_counter()
                for _ in range(reps):
                    run()
                side.synchronize()
                times[name].append((time.perf_counter() - t0) / (reps * G) * 1e6)
    return times


def report(times):
    return "  ".join(f"{name} {statistics.median(ts):7.2f} (spread {max(ts) - min(ts):5.2f})" for name, ts in times.items())


def measure_record(n, C):
    torch.manual_seed(0)
    comps = torch.randn((n, C), device=dev) * torch.logspace(-3, 2, C, device=dev)
    reward = comps.sum(1)
    done = (torch.rand(n, device=dev) < 0.01).to(torch.uint8)                       # an episode of about 100 steps
    mon, tm = RewardMonitor(n, ["t%d" % c for c in range(C)], capacity=CAPACITY), TorchMonitor(n, C, CAPACITY)
    label = f"{n:6d} x {C:2d}"
    for graph in (False, True):
        times = timed({"torch": lambda: tm.record(comps, reward, done), "device": lambda: mon.record(comps, reward, done)}, graph)
        t, d = times["torch"], times["device"]
        gap, spread = statistics.median(t) - statistics.median(d), max(max(t) - min(t), max(d) - min(d))
        say(f"{label}  record alone {'graph' if graph else 'eager'}: {report(times)}  us/record; device below torch by "
            f"{gap:7.2f} us (largest spread {spread:5.2f}): {'yes' if gap > spread else 'NO'}")
    # both saw the same stream of records: the device's row against torch's, as a check that the same thing was timed
    k = (mon.records - 1) % CAPACITY
    ours, theirs = mon.log[k].cpu(), tm.log[int((tm.records.item() - 1) % CAPACITY)].cpu()
    say(f"{label}  last row: largest |device - torch| {float((ours - theirs).abs().max()):.3e}; records {mon.records}, "
        f"episodes {mon.episode_stats(clear=False)['episodes']} (torch {int(tm.episodes.item())})")
    mon.close()


def measure_loop(n):
    torch.manual_seed(0)
    env = WalkingQuadrupedVecEnv(n, random_controls=True, random_init=True, device_commands=True,
                                 reset_options={"min_speed": 0.0, "max_speed": 0.5}, max_time=10.0, nan_direction=False)
    obs = torch.from_numpy(env.reset()).to(dev)
    raw, rew = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    done, comps = torch.zeros(n, device=dev, dtype=torch.uint8), torch.zeros((n, 11), device=dev)
    acts, logp, val, eps = torch.zeros((n, 12), device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros((n, 12), device=dev)
    pol = FusedMlpPolicy(33, (64, 64), 12, out_tanh=False, value=True)
    pol.set_params((0.1 * torch.randn(pol.n_params)).numpy())
    norm = RunningNormalizer(n, 33)
    buf = DeviceRolloutBuffer(n, 16, 33, 12)
    mon, tm = RewardMonitor.for_env(env, capacity=CAPACITY), TorchMonitor(n, 11, CAPACITY)
    buf.begin(obs)

    def base():
        eps.normal_()
        pol.forward(obs, acts, eps=eps, log_prob=logp, value=val)
        env.step_tensor(acts, obs, raw, done, components=comps)

    def rest():
        norm.step(obs, raw, done, reward_out=rew)
        buf.add(obs, acts, logp, val, rew, done, episode_reward=raw)                # (a full buffer stores nothing: the launch is the same)

    def bare():
        base(), rest()

    def with_device():
        base(), mon.record(comps, raw, done), rest()

    def with_torch():
        base(), tm.record(comps, raw, done), rest()

    label = f"{n:6d} x 11"
    for graph in (False, True):
        times = timed({"none": bare, "torch": with_torch, "device": with_device}, graph)
        med = {k: statistics.median(v) for k, v in times.items()}
        say(f"{label}  closed-loop step (policy, walking env, normaliser, rollout record) {'graph' if graph else 'eager'}: "
            f"{report(times)}  us/step; the monitor adds {med['device'] - med['none']:6.2f} us "
            f"({100 * (med['device'] - med['none']) / med['none']:4.1f} %), torch's {med['torch'] - med['none']:6.2f} us")
    ok = bool(torch.isfinite(mon.log).all())
    say(f"{label}  log finite {ok}; {mon.episode_stats(clear=False)['episodes']} episodes finished")
    for h in (mon, buf, norm, pol):
        h.close()
    env.close()


say(f"# tools/reward_monitor_rate.py: {G} records per graph, {args.rounds} alternated rounds of {args.steps} steps, median us; "
    f"build {_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
for shape in args.shapes:
    n, C = shape.split("x")
    measure_record(int(n), int(C))
if args.loop_envs > 0:
    measure_loop(args.loop_envs)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
