"""What the running normaliser (quadruped_gym_amd.normalize.RunningNormalizer, three launches per training step) costs against the same
step written in torch with float64 statistics, alone and in the closed loop beside the env step and the fused policy.  Shapes: the
plain step's packed [n, 35] rows in place (33 columns, stride 35: the 4-byte path) at 4096 envs, and the partially observed walking
step's 260 columns (the 16-byte path) at 4096 and 32 768 envs.  Each is run eagerly and as a hipGraph of 8 steps on one stream; the torch
and the device variants are timed in alternating rounds in this one process, the median of the rounds is reported with their spread
(max - min).  The normalise pass alone (training off, observations only, in place) gives the achieved bytes per second: 8 n D bytes
(one f32 read, one f32 write) over its time, as a fraction of the 8 TB/s HBM peak.

usage (GPU box): python tools/normalize_rate.py [--rounds 7] [--steps 800] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
from quadruped_gym_amd.normalize import RunningNormalizer
from quadruped_gym_amd.policy import FusedMlpPolicy
from quadruped_gym_amd.sim import BatchedSim

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=800)
ap.add_argument("--configs", nargs="+", default=["plain:4096", "po:4096", "po:32768"])
ap.add_argument("--out", default=None)
args = ap.parse_args()

G = 8
HBM_PEAK = 8e12
dev = torch.device("cuda:0")
GAMMA, EPS, CLIP = 0.99, 1e-8, 10.0
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


class TorchNormalizer:
    """The same step in torch: float64 statistics kept in device tensors (so a captured graph replays), elementwise passes in f64."""

    def __init__(self, n, D):
        f64 = dict(device=dev, dtype=torch.float64)
        self.n = n
        self.mean, self.var, self.count = torch.zeros(D, **f64), torch.ones(D, **f64), torch.full((), 1e-4, **f64)
        self.rmean, self.rvar, self.rcount = torch.zeros((), **f64), torch.ones((), **f64), torch.full((), 1e-4, **f64)
        self.returns = torch.zeros(n, **f64)

    @staticmethod
    def _update(mean, var, count, batch, n):
        bm, bv = batch.mean(0), batch.var(0, unbiased=False)
        delta, tot = bm - mean, count + n
        m2 = var * count + bv * n + delta * delta * count * n / tot
        mean.add_(delta * n / tot)
        var.copy_(m2 / tot)
        count.copy_(tot)

    def step(self, obs, rew, done):
        x = obs.double()
        self._update(self.mean, self.var, self.count, x, self.n)
        obs.copy_(((x - self.mean) / torch.sqrt(self.var + EPS)).clamp_(-CLIP, CLIP))
        r = rew.double()
        self.returns.mul_(GAMMA).add_(r)
        self._update(self.rmean, self.rvar, self.rcount, self.returns, self.n)
        rew.copy_((r / torch.sqrt(self.rvar + EPS)).clamp_(-CLIP, CLIP))
        self.returns.masked_fill_(done != 0, 0.0)


def timed(fn_by_name, graph):
    """Alternating rounds; returns {name: [us per step per round]}."""
    side = torch.cuda.Stream(dev)
    runs = {}
    for name, fn in fn_by_name.items():
        def loop(fn=fn):
            for k in range(G):
                fn(k)
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


def task():
    t = _abi.default_task()
    t.auto_reset, t.use_fall, t.fall_height = 1, 1, 0.05
    return t


def measure(kind, n):
    D = 33 if kind == "plain" else 260
    torch.manual_seed(0)
    acts, val = torch.zeros((n, 12), device=dev), torch.zeros(n, device=dev)
    pol = FusedMlpPolicy(D, (64, 64), 12, out_tanh=True, value=True)
    pol.set_params((0.1 * torch.randn(pol.n_params)).numpy())
    if kind == "plain":
        sim = BatchedSim(n, task=task())
        sim.reset(seed=0)
        rows = torch.zeros((n, D + 2), device=dev)
        obs, rew, done = rows[:, :D], rows[:, D], rows[:, D + 1]

        def env_step():
            sim.step_device_packed(acts, rows)
    else:
        env = POWalkingQuadrupedVecEnv(n, obs_window=10, random_controls=True, random_init=True, device_commands=True,
                                       reset_options={"min_speed": 0.0, "max_speed": 0.5}, settling_time=0.5, max_time=10.0,
                                       nan_direction=False)
        obs = torch.from_numpy(env.reset()).to(dev)
        rew, done = torch.zeros(n, device=dev), torch.zeros(n, device=dev, dtype=torch.uint8)

        def env_step():
            env.step_tensor(acts, obs, rew, done)
    raw = torch.randn((n, D), device=dev) * torch.logspace(-2, 1, D, device=dev) + 1.0
    tn, fn = TorchNormalizer(n, D), RunningNormalizer(n, D)
    label = f"{n:6d} x {D:3d} {'packed, in place' if kind == 'plain' else 'in place        '}"

    def normalise_torch(k):
        tn.step(obs, rew, done)

    def normalise_device(k):
        if kind == "plain":
            fn.step_packed(rows)
        else:
            fn.step(obs, rew, done)

    result = {}
    for with_env in (False, True):
        for graph in (False, True):
            variants = {}
            for name, norm in (("torch", normalise_torch), ("device", normalise_device)):
                if with_env:
                    def step(k, norm=norm):
                        pol.forward(obs, acts, value=val)
                        env_step()
                        norm(k)
                else:
                    def step(k, norm=norm):
                        norm(k)
                variants[name] = step
            if with_env:
                def bare(k):
                    pol.forward(obs, acts, value=val)
                    env_step()
                variants["none"] = bare
            else:
                obs.copy_(raw)                              # in place on its own output: finite, and the timing does not care
            times = timed(variants, graph)
            for name, ts in times.items():
                result[(name, with_env, graph)] = (statistics.median(ts), max(ts) - min(ts))
            what = "policy + env step + normalise" if with_env else "normalise alone              "
            text = "  ".join(f"{name} {statistics.median(ts):7.2f} (spread {max(ts) - min(ts):5.2f})" for name, ts in times.items())
            ok = bool(torch.isfinite(obs).all()) and bool(torch.isfinite(rew).all())
            say(f"{label}  {what} {'graph' if graph else 'eager'}: {text}  us/step  finite {ok}")
    for graph in (False, True):
        t, f = result[("torch", False, graph)], result[("device", False, graph)]
        spread = max(t[1], f[1])
        say(f"{label}  {'graph' if graph else 'eager'}: device below torch by {t[0] - f[0]:7.2f} us (largest spread {spread:5.2f} us): "
            f"{'yes' if t[0] - f[0] > spread else 'NO'}; in the loop {result[('none', True, graph)][0]:7.2f} bare, "
            f"{result[('torch', True, graph)][0]:7.2f} torch, {result[('device', True, graph)][0]:7.2f} device us/step")

    # the normalise pass alone: training off, observations only, in place
    fn.training = False
    buf = raw.clone() if kind != "plain" else rows
    view = buf if kind != "plain" else rows[:, :D]
    times = timed({"apply": lambda k: fn.normalize_obs(view)}, True)["apply"]
    us = statistics.median(times)
    rate = 8.0 * n * D / (us * 1e-6)
    say(f"{label}  normalise pass alone (graph): {us:7.2f} us (spread {max(times) - min(times):5.2f}), {8 * n * D / 1e6:7.2f} MB -> "
        f"{rate / 1e12:5.2f} TB/s, {100 * rate / HBM_PEAK:5.1f} % of 8 TB/s")
    fn.close()
    pol.close()
    if kind == "plain":
        sim.close()
    else:
        env.close()


say(f"# tools/normalize_rate.py: {G} steps per graph, {args.rounds} alternated rounds of {args.steps} steps, median us/step; "
    f"build {_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
for cfg in args.configs:
    kind, n = cfg.split(":")
    measure(kind, int(n))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
