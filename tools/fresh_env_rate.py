"""QuadrupedVecEnv.step at 32768 envs as tools/host_path_rate.py builds and times it, but in a process that has run nothing else
(or, with `history`, one POWalkingQuadrupedVecEnv of 4096 envs): time and minor page faults per step.  What the heap holds when the
env is built decides whether glibc keeps the pages of the per-step output arrays.  usage: python tools/fresh_env_rate.py [history]"""
import os
import resource
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (loads the HIP runtime the library links against)
from quadruped_gym_amd.envs.vec_env import QuadrupedVecEnv  # noqa: E402
from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv  # noqa: E402


def faults():
    return resource.getrusage(resource.RUSAGE_SELF).ru_minflt


def rate(env, acts, m, label):
    env.reset()
    for k in range(5):
        env.step(acts[k & 7])
    f0, t0 = faults(), time.perf_counter()
    for k in range(m):
        env.step(acts[k & 7])
    dt, f = time.perf_counter() - t0, faults() - f0
    print(f"{label}: {dt / m * 1e6:8.1f} us/step, {f / m:8.1f} minor page faults per step")


history = len(sys.argv) > 1
rng = np.random.default_rng(0)
env = None
if history:
    small = [rng.uniform(-1, 1, (4096, 12)).astype(np.float32) for _ in range(8)]
    env = POWalkingQuadrupedVecEnv(4096, obs_window=10)
    rate(env, small, 100, "history: POWalkingQuadrupedVecEnv(4096, w10)")
    env.close()
acts = [rng.uniform(-1, 1, (32768, 12)).astype(np.float32) for _ in range(8)]
env = QuadrupedVecEnv(32768, reward_fns={"forward": 1.0, "control_cost": -0.1, "alive_bonus": 1.0}, termination_fns={"fall": 0.05})
rate(env, acts, 40, "QuadrupedVecEnv(32768)" + (" after the history" if history else " alone"))
env.close()
