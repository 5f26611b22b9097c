"""What the GPU tests of the fused MLP policy share (tests/test_policy_gpu.py, tests/test_policy_shapes_gpu.py,
tests/test_ppo_iteration_gpu.py): the device, the forward pass's tolerance rule, the torch float32 tower it is measured against, and
the record file.  Nothing here runs on the GPU at import."""
import os

import numpy as np
import torch

DEV = "cuda:0"


def record(line):
    print(line)
    out = os.environ.get("QG_POLICY_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def bound(torch_err, ref):
    """The fused kernel's maximum absolute error may be at most 4x the torch float32 path's on the same inputs, with a floor of 1e-6."""
    return max(4.0 * torch_err, 1e-6)


def observations(rng, n, obs_dim):
    """Per-column scales from 0.01 to 10."""
    return (rng.standard_normal((n, obs_dim)) * np.logspace(-2, 1, obs_dim)).astype(np.float32)


def torch_tower(layers, out_tanh):
    mods = []
    for k, (W, b) in enumerate(layers):
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W))
            lin.bias.copy_(torch.from_numpy(b))
        mods.append(lin)
        if k < len(layers) - 1 or out_tanh:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods).to(DEV)


def run(pol, obs_t, eps_t=None, want_lp=True):
    n = obs_t.shape[0]
    act = torch.full((n, pol.act_dim), float("nan"), device=DEV)
    lp = torch.full((n,), float("nan"), device=DEV) if want_lp else None
    val = torch.full((n,), float("nan"), device=DEV) if pol.has_value else None
    pol.forward(obs_t, act, eps=eps_t, log_prob=lp, value=val)
    torch.cuda.synchronize()
    return act.cpu().numpy(), (lp.cpu().numpy() if want_lp else None), (val.cpu().numpy() if val is not None else None)
