"""What the command curriculum costs behind the env-step at 4096 and 32 768 envs, around the walking env and the partially observable
env at obs_window = 10: the two launches of csrc/qg_cmdcur.hip against the env-step with the in-kernel sampler (what the step costs
where commands are drawn uniformly inside it) and against the closest torch expression of the same curriculum.

  step:               env.step_tensor(actions, obs, reward, done, components)          fixed commands: the env-step alone
  step+advance:  (a)  ... then curriculum.step(done, components, command_out): TWO launches
  sampler step:  (b)  the same env built with random_controls=True, device_commands=True: the step kernels' own uniform sampler
  step+torch:    (c)  ... then the curriculum in torch: the criteria's sums, the judgement, the successes per bin (index_add_: bincount
                      with a minlength waits for the device, which a graph cannot hold), the neighbour sums by shifted adds, cumsum,
                      rand and searchsorted, the new commands by torch.where; eagerly followed by the host round trip of
                      env.set_commands, which is the only way such commands reach the walking layer.  Under a graph the round trip is
                      left out -- in torch's favour: those commands never reach the step.

Each side is timed eagerly (host clock around `reps` calls that end in a synchronise) and as a hipGraph of one call (torch.cuda.graph),
all sides in alternating rounds in this one process on the same build; the median of the rounds is reported with their spread
(max - min).  The method is tools/gait_schedule_rate.py's.

usage (GPU box): python tools/command_curriculum_rate.py [--rounds 5] [--reps 300] [--out FILE]"""
import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.curriculum import CommandCurriculum, initial_weights_for
from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv, WalkingQuadrupedVecEnv

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--torch-reps", type=int, default=40)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
SIZES = (4096, 32768)
SPEED, BINS, W, DELTA, R, MIN_STEPS = (0.0, 1.0), (8, 8), 64, 8, 50, 10
CRITERIA = ((2, 1, 0.0), (1, -1, 0.0))                   # progress_direction_reward_local's mean >= 0, control_cost's <= 0
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def time_sides(sides, graphable):
    """``{(mode, name): (median us/call, spread)}`` of the callables ``sides``, eagerly and as a graph of one call (``graphable[name]``
    is what the graph holds: the side itself, or its part a graph can hold)."""
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        for fn in list(sides.values()) + list(graphable.values()):
            for _ in range(3):
                fn()
    side.synchronize()
    graphs = {}
    for name, fn in graphable.items():
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
                for _ in range(10):
                    call()
            side.synchronize()
            for _ in range(args.rounds):
                for name, call in calls.items():         # alternated: one round of each in turn
                    reps = args.torch_reps if (mode == "eager" and name == "step+torch") else args.reps
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        call()
                    side.synchronize()
                    times[name].append((time.perf_counter() - t0) / reps * 1e6)
        for name, ts in times.items():
            result[(mode, name)] = (statistics.median(ts), max(ts) - min(ts))
    del graphs
    return result


def measure(kind, n):
    make = (lambda **kw: WalkingQuadrupedVecEnv(n, nan_direction=False, **kw)) if kind == "walking" else \
           (lambda **kw: POWalkingQuadrupedVecEnv(n, obs_window=10, nan_direction=False, **kw))
    env, sampled = make(), make(random_controls=True, device_commands=True, reset_options={"min_speed": SPEED[0], "max_speed": SPEED[1]})
    env.reset(), sampled.reset()
    O, B = env.obs_dim, BINS[0] * BINS[1]
    initial = initial_weights_for(SPEED, BINS, (0.0, 0.25), W)
    cur = CommandCurriculum(env._walk, SPEED, BINS, initial, W, DELTA, R, MIN_STEPS, CRITERIA, seed=1)
    actions = torch.tensor([0.0, 0.0, -0.5] * 4, device=dev).repeat(n, 1).contiguous()
    bufs = [(torch.zeros((n, O), device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev, dtype=torch.uint8),
             torch.zeros((n, 11), device=dev)) for _ in range(2)]
    (obs, reward, done, comps), other = bufs
    out = torch.zeros((n, 4), device=dev)
    for _ in range(150):                                     # the robots settle on their feet
        env.step_tensor(actions, obs, reward, done, comps)
        sampled.step_tensor(actions, *other)
    # the torch side's state
    weight = torch.from_numpy(initial.astype("int64")).to(dev)
    bins = torch.zeros(n, dtype=torch.int64, device=dev)
    steps, sums = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros((n, 2), device=dev)
    cmd = torch.zeros((n, 4), device=dev)
    cols = torch.tensor([c for c, _, _ in CRITERIA], device=dev)
    sense = torch.tensor([float(s) for _, s, _ in CRITERIA], device=dev)
    thr = torch.tensor([t for _, _, t in CRITERIA], device=dev)
    ws, wa = (SPEED[1] - SPEED[0]) / BINS[0], 2 * math.pi / BINS[1]

    def step():
        env.step_tensor(actions, obs, reward, done, comps)

    def advance():
        env.step_tensor(actions, obs, reward, done, comps)
        cur.step(done, comps, out)

    def sampler():
        sampled.step_tensor(actions, *other)

    def torch_device():
        env.step_tensor(actions, obs, reward, done, comps)
        steps.add_(1)
        sums.add_(comps[:, cols])
        ended = (done != 0) | (steps == R)
        ok = ended & (steps >= MIN_STEPS) & ((sense * (sums - thr * steps.unsqueeze(1).float())) >= 0).all(1)
        s_b = torch.zeros(B, dtype=torch.int64, device=dev).index_add_(0, bins, ok.long()).view(BINS)
        gain = s_b + torch.roll(s_b, 1, 1) + torch.roll(s_b, -1, 1)
        gain[1:] += s_b[:-1]
        gain[:-1] += s_b[1:]
        weight.copy_(torch.clamp(weight + DELTA * gain.view(-1), max=W))
        cdf = torch.cumsum(weight, 0)
        u = torch.rand((4, n), device=dev)
        new = torch.searchsorted(cdf, (u[0] * cdf[-1]).long(), right=True).clamp_(max=B - 1)
        speed = SPEED[0] + ((new // BINS[1]).float() + u[1]) * ws
        alpha = -math.pi + ((new % BINS[1]).float() + u[2]) * wa
        theta = math.pi * (2 * u[3] - 1)
        fresh = torch.stack([speed * torch.cos(alpha), speed * torch.sin(alpha), torch.cos(theta), torch.sin(theta)], dim=1)
        cmd.copy_(torch.where(ended.unsqueeze(1), fresh, cmd))
        bins.copy_(torch.where(ended, new, bins))
        steps.masked_fill_(ended, 0)
        sums.masked_fill_(ended.unsqueeze(1), 0.0)

    def torch_full():
        torch_device()
        host = cmd.cpu().numpy()
        env.set_commands(host[:, :2], host[:, 2:])

    sides = {"step": step, "step+advance": advance, "sampler step": sampler, "step+torch": torch_full}
    result = time_sides(sides, dict(sides, **{"step+torch": torch_device}))
    for mode in ("eager", "graph"):
        s, a, b, c = (result[(mode, k)] for k in ("step", "step+advance", "sampler step", "step+torch"))
        say(f"{kind:7s} {O:3d} cols {n:6d} envs  {mode:5s}: step {s[0]:6.1f} (spread {s[1]:4.1f})   (a) step+advance {a[0]:6.1f} (spread {a[1]:4.1f})   "
            f"(b) sampler step {b[0]:6.1f} (spread {b[1]:4.1f})   (c) step+torch {c[0]:7.1f} (spread {c[1]:5.1f}) us   "
            f"advance adds {a[0] - s[0]:5.1f} us, the sampler {b[0] - s[0]:5.1f} us, torch {c[0] - s[0]:7.1f} us")
    stats = cur.stats()
    say(f"        ({int(stats['episodes'].sum())} segments judged on the way, {int((cur.weights() > 0).sum())} of {B} bins unlocked)")
    cur.close()
    env.close(), sampled.close()


say(f"# tools/command_curriculum_rate.py: {args.rounds} alternated rounds of {args.reps} calls ({args.torch_reps} for the eager torch side), "
    f"median us per call; build {_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
for kind in ("walking", "po"):
    for n in SIZES:
        measure(kind, n)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
