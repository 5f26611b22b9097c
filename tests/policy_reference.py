"""Float64 restatement of the fused policy's forward pass (include/quadgym.h, "fused MLP policy"), written from the formulae and not
from the kernel: the checker of tests/test_policy_api.py and tests/test_policy_gpu.py.  NumPy only."""
import math

import numpy as np

# the three shapes the measurements and tests use: (obs_dim, hidden, act_dim)
SHAPES = {
    "plain": (33, (64, 64), 12),             # the plain step's 33-value observation, SB3's MlpPolicy default
    "po": (260, (64, 64), 12),               # the partially observed walking stack, same body
    "po_wide": (260, (256, 256, 128), 12),   # the reference's net_arch
}


def tower_shapes(obs_dim, hidden, out_dim):
    dims = (obs_dim,) + tuple(hidden)
    return [(dims[i + 1], dims[i]) for i in range(len(hidden))] + [(out_dim, dims[-1])]


def param_count(obs_dim, hidden, act_dim, value):
    count = sum(o * i + o for o, i in tower_shapes(obs_dim, hidden, act_dim)) + act_dim
    if value:
        count += sum(o * i + o for o, i in tower_shapes(obs_dim, hidden, 1))
    return count


def random_layers(rng, shapes, init="sb3", head_gain=0.01):
    """Asymmetric random weights.  ``sb3``: orthogonal, gain sqrt(2) on hidden layers and ``head_gain`` on the last, small random
    biases (SB3 zeroes them; zeros would hide a misplaced bias); ``linear``: torch.nn.Linear's default U(-1/sqrt(in), 1/sqrt(in))."""
    layers = []
    for k, (o, i) in enumerate(shapes):
        if init == "sb3":
            a = rng.standard_normal((max(o, i), min(o, i)))
            q, r = np.linalg.qr(a)
            q = q * np.sign(np.diag(r))
            W = (q if o >= i else q.T) * (math.sqrt(2.0) if k < len(shapes) - 1 else head_gain)
            b = rng.uniform(-0.1, 0.1, o)
        else:
            bound = 1.0 / math.sqrt(i)
            W = rng.uniform(-bound, bound, (o, i))
            b = rng.uniform(-bound, bound, o)
        layers.append((W.astype(np.float32), b.astype(np.float32)))
    return layers


def flatten(actor, log_std, critic=None):
    """Canonical flat vector: actor layers (W row-major, b), log_std, critic layers."""
    parts = []
    for W, b in actor:
        parts += [np.asarray(W, np.float32).ravel(), np.asarray(b, np.float32).ravel()]
    parts.append(np.asarray(log_std, np.float32).ravel())
    for W, b in (critic or []):
        parts += [np.asarray(W, np.float32).ravel(), np.asarray(b, np.float32).ravel()]
    return np.concatenate(parts)


def mlp(layers, x, out_tanh):
    h = np.asarray(x, np.float64)
    for k, (W, b) in enumerate(layers):
        h = h @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)
        if k < len(layers) - 1 or out_tanh:
            h = np.tanh(h)
    return h


def forward(actor, log_std, obs, eps=None, critic=None, out_tanh=False):
    """``(mean, action, log_prob, value)`` in float64; ``eps=None`` is the deterministic action (eps = 0 in the log-density)."""
    mean = mlp(actor, obs, out_tanh)
    ls = np.asarray(log_std, np.float64)
    e = np.zeros_like(mean) if eps is None else np.asarray(eps, np.float64)
    action = mean + np.exp(ls) * e
    log_prob = (-0.5 * e * e - ls - 0.5 * math.log(2.0 * math.pi)).sum(-1)
    value = mlp(critic, obs, False)[:, 0] if critic else None
    return mean, action, log_prob, value
