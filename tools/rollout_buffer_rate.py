"""What the device rollout buffer (quadruped_gym_amd.rollout.DeviceRolloutBuffer, one launch per call) costs against the torch code it
replaces.  Four measurements, the variants of each timed in alternating rounds in this one process; the median of the rounds is
reported with their spread (max - min), in microseconds per call:

  1. add      the record of a step from the plain env's packed [n, 35] rows at 4096 envs, against the six torch copies that write
              obs[k + 1], actions[k], log_probs[k], values[k], rewards[k], dones[k] (they keep no episode statistics); eagerly and as a
              hipGraph of 8 steps.  Both start every 8 steps at slot 0 (the device buffer through begin(), whose launch is in its figure).
  2. compute  GAE over K filled slots against the backward loop in torch (SB3's order), K = 16, 128, 2048 at 4096 envs and K = 16 at
              32 768 (buffers with obs_dim = act_dim = 1: the pass does not touch the observations); the torch loop also as a hipGraph
              up to K = 128.
  3. gather   a minibatch of B = 4096 and 65 536 rows of 33 + 12 + 4 floats out of 16 x 4096 samples against six index_selects into
              preallocated outputs; eagerly and as a hipGraph of 8.
  4. loop     fused 64-64 policy with critic + env step + normaliser at 4096 envs (the loop of DESIGN 4.9's table) bare, with the
              torch copies and with the buffer's add.

usage (GPU box): python tools/rollout_buffer_rate.py [--rounds 7] [--steps 800] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.normalize import RunningNormalizer
from quadruped_gym_amd.policy import FusedMlpPolicy
from quadruped_gym_amd.rollout import DeviceRolloutBuffer
from quadruped_gym_amd.sim import BatchedSim

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--steps", type=int, default=800)
ap.add_argument("--skip", nargs="*", default=[], choices=["add", "compute", "gather", "loop"])
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert args.rounds >= 7, "the median of at least seven alternated rounds"

G = 8
dev = torch.device("cuda:0")
GAMMA, LAM = 0.99, 0.95
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(groups, graph, calls_per_group, reps):
    """groups: {name: function that enqueues one group of calls}.  Alternating rounds; {name: (median, spread)} in us per call."""
    side = torch.cuda.Stream(dev)
    runs = {}
    for name, fn in groups.items():
        with torch.cuda.stream(side):
            fn()
        side.synchronize()
        if graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                fn()
            runs[name] = g.replay
        else:
            runs[name] = fn
    times = {name: [] for name in runs}
    with torch.cuda.stream(side):
        for run in runs.values():
            for _ in range(min(10, reps)):
                run()
        side.synchronize()
        for _ in range(args.rounds):
            for name, run in runs.items():
                t0 = time.perf_counter()
                for _ in range(reps):
                    run()
                side.synchronize()
                times[name].append((time.perf_counter() - t0) / (reps * calls_per_group) * 1e6)
    return {name: (statistics.median(ts), max(ts) - min(ts)) for name, ts in times.items()}


def fmt(res):
    return "  ".join(f"{name} {m:9.2f} (spread {s:7.2f})" for name, (m, s) in res.items())


class TorchStorage:
    """The [K, n] buffers and the per-step copies the INTEGRATION examples write by hand."""

    def __init__(self, n, K, D, A):
        f32 = dict(device=dev, dtype=torch.float32)
        self.obs, self.actions = torch.zeros((K + 1, n, D), **f32), torch.zeros((K, n, A), **f32)
        self.log_probs, self.values, self.rewards = torch.zeros((K, n), **f32), torch.zeros((K, n), **f32), torch.zeros((K, n), **f32)
        self.dones = torch.zeros((K, n), device=dev, dtype=torch.uint8)
        self.advantages, self.returns = torch.zeros((K, n), **f32), torch.zeros((K, n), **f32)
        self.D = D

    def add(self, k, rows, acts, logp, val):
        D = self.D
        self.obs[k + 1].copy_(rows[:, :D])
        self.actions[k].copy_(acts)
        self.log_probs[k].copy_(logp)
        self.values[k].copy_(val)
        self.rewards[k].copy_(rows[:, D])
        self.dones[k].copy_(rows[:, D + 1])

    def compute(self, last_values):
        """RolloutBuffer.compute_returns_and_advantage, with dones[t] for episode_starts[t + 1]."""
        K = self.rewards.shape[0]
        gae = torch.zeros_like(last_values)
        for t in range(K - 1, -1, -1):
            nnt = 1.0 - self.dones[t].float()
            nv = last_values if t == K - 1 else self.values[t + 1]
            delta = self.rewards[t] + GAMMA * nv * nnt - self.values[t]
            gae = delta + GAMMA * LAM * nnt * gae
            self.advantages[t] = gae
        torch.add(self.advantages, self.values, out=self.returns)


def measure_add(n=4096, D=33, A=12):
    rows = torch.randn((n, D + 2), device=dev)
    rows[:, D + 1] = (torch.rand(n, device=dev) < 0.02).float()
    acts, logp, val = torch.randn((n, A), device=dev), torch.randn(n, device=dev), torch.randn(n, device=dev)
    buf, ts = DeviceRolloutBuffer(n, G, D, A), TorchStorage(n, G, D, A)

    def device():
        buf.begin(rows[:, :D])
        for k in range(G):
            buf.add_packed(rows, acts, logp, val)

    def torch_copies():
        ts.obs[0].copy_(rows[:, :D])
        for k in range(G):
            ts.add(k, rows, acts, logp, val)

    for graph in (False, True):
        res = timed({"torch": torch_copies, "device": device}, graph, G, max(1, args.steps // G))
        say(f"add      {n:6d} x {D} packed, {'graph' if graph else 'eager'}: {fmt(res)}  us/step")
    info = buf.info()
    assert info["pos"] == G and info["overflow"] == 0 and torch.equal(buf.observations[1:], ts.obs[1:]) and torch.equal(buf.dones, ts.dones)
    buf.close()


def measure_compute(n, K):
    buf, ts = DeviceRolloutBuffer(n, K, 1, 1, gamma=GAMMA, gae_lambda=LAM), TorchStorage(n, K, 1, 1)
    row, z = torch.zeros((n, 1), device=dev), torch.zeros(n, device=dev)
    buf.begin(row)
    for k in range(K):
        buf.add(row, row, z, z, z, z)                       # moves the cursor to K; the storage is rewritten below
    for t in (buf, ts):
        t.rewards.normal_(), t.values.normal_().mul_(3.0)
        t.dones.copy_(torch.rand((K, n), device=dev) < 0.02)
    ts.rewards.copy_(buf.rewards), ts.values.copy_(buf.values), ts.dones.copy_(buf.dones)
    lv = 3.0 * torch.randn(n, device=dev)
    reps = max(1, min(args.steps, 4096 // K))
    res = timed({"torch": lambda: ts.compute(lv), "device": lambda: buf.compute_returns_and_advantage(lv)}, False, 1, reps)
    say(f"compute  {n:6d} envs, K = {K:4d}, eager: {fmt(res)}  us/pass")
    if K <= 128:
        res = timed({"torch": lambda: ts.compute(lv), "device": lambda: buf.compute_returns_and_advantage(lv)}, True, 1, reps)
        say(f"compute  {n:6d} envs, K = {K:4d}, graph: {fmt(res)}  us/pass")
    torch.cuda.synchronize()
    err = float((buf.advantages - ts.advantages).abs().max())
    say(f"compute  {n:6d} envs, K = {K:4d}: largest |device - torch| advantage {err:.3g}; bytes moved {17 * n * K / 1e6:.1f} MB")
    buf.close()


def measure_gather(n=4096, K=16, D=33, A=12):
    buf, ts = DeviceRolloutBuffer(n, K, D, A), TorchStorage(n, K, D, A)
    rows = torch.randn((n, D + 2), device=dev)
    acts, logp, val = torch.randn((n, A), device=dev), torch.randn(n, device=dev), torch.randn(n, device=dev)
    buf.begin(rows[:, :D])
    for k in range(K):
        buf.add_packed(rows, acts, logp, val)
    buf.compute_returns_and_advantage(val)
    total = K * n
    flat = [buf.observations[:K].reshape(total, D), buf.actions.reshape(total, A), buf.values.reshape(total), buf.log_probs.reshape(total),
            buf.advantages.reshape(total), buf.returns.reshape(total)]
    for B in (4096, 65536):
        idx = [torch.randperm(total, device=dev)[:B].contiguous() for _ in range(G)]
        outs = [torch.empty((B,) + tuple(f.shape[1:]), device=dev) for f in flat]

        def torch_selects():
            for k in range(G):
                for f, o in zip(flat, outs):
                    torch.index_select(f, 0, idx[k], out=o)

        def device():
            for k in range(G):
                buf.sample(idx[k])

        for graph in (False, True):
            res = timed({"torch": torch_selects, "device": device}, graph, G, max(1, args.steps // G))
            say(f"gather   B = {B:6d} of {total} samples x ({D} + {A} + 4) floats, {'graph' if graph else 'eager'}: {fmt(res)}  us/batch")
        got = buf.sample(idx[G - 1])
        torch.cuda.synchronize()
        assert all(torch.equal(g, o) for g, o in zip(got, outs)) and buf.info()["bad_index"] == 0
    buf.close()


def measure_loop(n=4096, D=33, A=12):
    task = _abi.default_task()
    task.auto_reset, task.use_fall, task.fall_height = 1, 1, 0.05
    sim = BatchedSim(n, task=task)
    sim.reset(seed=0)
    torch.manual_seed(0)
    pol = FusedMlpPolicy(D, (64, 64), A, out_tanh=True, value=True)
    pol.set_params((0.1 * torch.randn(pol.n_params)).numpy())
    nz = RunningNormalizer(n, D)
    rows = torch.zeros((n, D + 2), device=dev)
    acts, logp, val = torch.zeros((n, A), device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    buf, ts = DeviceRolloutBuffer(n, G, D, A), TorchStorage(n, G, D, A)

    def step():
        pol.forward(rows[:, :D], acts, log_prob=logp, value=val)
        sim.step_device_packed(acts, rows)
        nz.step_packed(rows)

    def bare():
        for k in range(G):
            step()

    def with_torch():
        ts.obs[0].copy_(rows[:, :D])
        for k in range(G):
            step()
            ts.add(k, rows, acts, logp, val)

    def with_buffer():
        buf.begin(rows[:, :D])
        for k in range(G):
            step()
            buf.add_packed(rows, acts, logp, val)

    for graph in (False, True):
        res = timed({"bare": bare, "torch": with_torch, "buffer": with_buffer}, graph, G, max(1, args.steps // G))
        say(f"loop     {n:6d} x {D}: policy + env step + normalise, {'graph' if graph else 'eager'}: {fmt(res)}  us/step")
    assert buf.info()["pos"] == G and bool(torch.isfinite(buf.observations).all())
    for h in (buf, nz, pol, sim):
        h.close()


say(f"# tools/rollout_buffer_rate.py: {G} calls per graph, {args.rounds} alternated rounds of {args.steps} steps, median us per call "
    f"(spread = max - min over the rounds); build {_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
if "add" not in args.skip:
    measure_add()
if "compute" not in args.skip:
    for n_, K_ in ((4096, 16), (4096, 128), (4096, 2048), (32768, 16)):
        measure_compute(n_, K_)
if "gather" not in args.skip:
    measure_gather()
if "loop" not in args.skip:
    measure_loop()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
