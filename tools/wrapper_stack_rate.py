"""What one ``step_tensor`` of INTEGRATION.md section 20's stack costs -- DeviceVecNormalize(DevicePrivilegedVecEnv(DevicePerturbedVecEnv(
POWalkingQuadrupedVecEnv))) at 4096 envs, obs_window 10 -- with ``terminal_obs=None`` (the training hot path: perturb_actions, the
env's launch, observe, the pack launch, the normaliser's three) and with a ``terminal_obs`` buffer (the terminal rows normalised with
the leading columns of the statistics, through the wrapper's wide scratch).

Each side is timed eagerly on a side stream (host clock around `reps` calls that end in a synchronise), the sides in alternating
rounds in this one process; the median of the rounds is reported with their spread (max - min).  A side the build cannot run (a
terminal_obs narrower than the normaliser before the wrapper took one) is reported as refused.

usage (GPU box): python tools/wrapper_stack_rate.py [--envs 4096] [--rounds 7] [--reps 300] [--hot-only] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
from quadruped_gym_amd.normalize import DeviceVecNormalize
from quadruped_gym_amd.perturb import DevicePerturbedVecEnv
from quadruped_gym_amd.privileged import DevicePrivilegedVecEnv

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=300)
ap.add_argument("--hot-only", action="store_true", help="time the terminal_obs=None side alone")
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
n = args.envs
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


env = POWalkingQuadrupedVecEnv(n, obs_window=10, random_controls=True, device_commands=True, nan_direction=False)
env = DevicePerturbedVecEnv(env, obs_noise={"gyro": 0.05}, action_latency=(0.0, 0.016), seed=1)
env = DevicePrivilegedVecEnv(env, force_threshold=1.0)
env = DeviceVecNormalize(env)
O, W = env.actor_obs_dim, env.obs_dim
env.reset()
actions = torch.tensor([0.0, 0.0, -0.5] * 4, device=dev).repeat(n, 1).contiguous()
obs, reward, done = torch.zeros((n, W), device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev, dtype=torch.uint8)
term = torch.zeros((n, O), device=dev)

sides = {"terminal_obs=None": lambda: env.step_tensor(actions, obs, reward, done),
         "terminal_obs [N, %d]" % O: lambda: env.step_tensor(actions, obs, reward, done, terminal_obs=term)}
if args.hot_only:
    sides = {"terminal_obs=None": sides["terminal_obs=None"]}
say(f"# tools/wrapper_stack_rate.py: normalise(privileged(perturb(PO env))), {n} envs x {W} columns, {args.rounds} alternated rounds of "
    f"{args.reps} calls, median us per step_tensor; build {_abi.load_library().qg_build_id().decode()}; {torch.cuda.get_device_name(0)}")
side = torch.cuda.Stream(dev)
with torch.cuda.stream(side):
    for name in list(sides):
        try:
            for _ in range(20):
                sides[name]()
        except ValueError as err:
            say(f"{name:22s}: refused ({str(err)[:100]})")
            del sides[name]
            env.reset()
    side.synchronize()
    times = {name: [] for name in sides}
    for _ in range(args.rounds):
        for name, call in sides.items():
            t0 = time.perf_counter()
            for _ in range(args.reps):
                call()
            side.synchronize()
            times[name].append((time.perf_counter() - t0) / args.reps * 1e6)
for name, ts in times.items():
    say(f"{name:22s}: {statistics.median(ts):7.1f} us per step (spread {max(ts) - min(ts):5.1f}) = {n / statistics.median(ts):6.1f} M env-steps/s")
env.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
