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


# Descriptions chosen against the forward kernel's branches: every launch shape meets an idle wave, a one-block wave, a
# partly filled and a full wave where it can have them, every class of its chunk loop, and the obs_dim / act_dim / LDS edges.
# tests/test_policy_api.py holds the census that pins this; tests/test_policy_shapes_gpu.py runs every row at one and four waves.
SHAPE_TABLE = (
    # widest layer <= 64: <4,1> and <1,4>
    (1, (16,), 1), (3, (32,), 3), (16, (48,), 4), (17, (64,), 5), (33, (16, 64), 12), (63, (64, 16), 13),
    (64, (48, 32, 16), 16), (65, (16, 16, 16), 2), (512, (64, 64, 64), 12), (260, (32, 48), 7),
    (40, (16, 48, 64), 8),        # third hidden layer wider than the first: it sizes LDS buffer 1
    # wider: <4,4> and <1,16>
    (1, (80,), 1), (15, (128,), 16), (33, (144,), 12), (100, (192,), 6), (260, (208,), 12), (511, (256,), 9),
    (5, (16, 256), 12), (260, (256, 16), 3), (48, (80, 256, 48), 12), (129, (240, 96, 176), 15),
    (512, (256, 256, 256), 16), (20, (16, 32, 240), 4), (257, (112, 224), 1),
)

TILE = 16                        # envs per workgroup


def launch_shape(hidden, n, towers, simds, force_waves=0):
    """``(waves per env tile, output blocks per wave)`` by the rule of DESIGN 4.8: four waves for nets wider than 64 at every size and
    for the narrow ones while tiles x towers is below the SIMD count, one from there on (``force_waves``: QG_POLICY_WAVES); a wave
    holds 1 / 4 blocks on four waves and 4 / 16 on one, by whether the widest layer fits 64."""
    widest = max(hidden)
    tiles = -(-n // TILE)
    waves = force_waves if force_waves in (1, 4) else (4 if widest > 64 or tiles * towers < simds else 1)
    narrow = widest <= 64
    return waves, {4: 1 if narrow else 4, 1: 4 if narrow else 16}[waves]


def conditions(desc, waves):
    """The branch conditions of the forward pass that ``desc = (obs_dim, hidden, act_dim)`` exercises when launched with ``waves``
    waves per tile: a set of ``(waves, blocks, name)``.

    Per hidden layer (a wave ``w`` of ``W`` owns the output blocks ``w, w + W, ..`` of the layer's ``nb``; it runs ``blocks``
    accumulators): ``hidden:idle`` a wave with no block, ``hidden:single`` one block on a wave that has several accumulators (the
    one-accumulator path), ``hidden:partial`` more than one block but not all accumulators (the rest run on clamped weights and are
    not stored), ``hidden:full``, and ``hidden:uneven`` when the busy waves of one layer hold different counts.
    Per layer, the output layer included, with ``nq`` input blocks of 16 and a chunk loop that advances by two half-chunks of
    ``kq = 16 / blocks`` input blocks: ``chunk:nq<kq``, ``chunk:second-half-off`` (the last round's second half-chunk entirely guarded
    off), ``chunk:multiple`` (``nq`` a multiple of ``2 kq``), ``chunk:second-half-partial`` (``nq % 2 kq > kq``) and ``chunk:rounds>1``.
    And the edges of the description itself: ``obs:no-padding``, ``obs<4``, ``obs=512``, ``act:partial-group``, ``act<4``,
    ``lds1:hidden2`` (buffer 1 sized by the third hidden layer), ``lds0:hidden1`` (buffer 0 by the second, not by the observation)."""
    obs_dim, hidden, act_dim = desc
    _, blocks = launch_shape(hidden, 1, 1, 1, force_waves=waves)
    kq = 16 // blocks
    names = set()
    for h in hidden:
        nb = h // 16
        counts = [len(range(w, nb, waves)) for w in range(waves)]
        for c in counts:
            if c == 0:
                names.add("hidden:idle")
            elif c == 1 and blocks > 1:
                names.add("hidden:single")
            elif c < blocks:
                names.add("hidden:partial")
            else:
                assert c == blocks
                names.add("hidden:full")
        if len({c for c in counts if c}) > 1:
            names.add("hidden:uneven")
    for width in (obs_dim,) + tuple(hidden):
        nq = -(-width // 16)
        rest = nq % (2 * kq)
        if nq < kq:
            names.add("chunk:nq<kq")
        if rest == 0:
            names.add("chunk:multiple")
        elif rest <= kq:
            names.add("chunk:second-half-off")
        else:
            names.add("chunk:second-half-partial")
        if nq > 2 * kq:
            names.add("chunk:rounds>1")
    if obs_dim % 16 == 0:
        names.add("obs:no-padding")
    if obs_dim < 4:
        names.add("obs<4")
    if obs_dim == 512:
        names.add("obs=512")
    if act_dim % 4:
        names.add("act:partial-group")
    if act_dim < 4:
        names.add("act<4")
    if len(hidden) > 2 and hidden[2] > hidden[0]:
        names.add("lds1:hidden2")
    if len(hidden) > 1 and hidden[1] > 16 * -(-obs_dim // 16):
        names.add("lds0:hidden1")
    return {(waves, blocks, name) for name in names}


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
