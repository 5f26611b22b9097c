"""The asymmetric actor-critic's PPO loss and gradient in float64, COMPOSED from tests/ppo_reference.py: the policy part on the actor's
columns [0, O) of the wide rows with no critic, the value part on the critic's window [offset, offset + dim) of the same rows; the
gradient is the concatenation in the canonical order (actor layers, log_std, critic layers).  tests/test_asym_critic_reference.py
holds it against torch float64 autograd of the loss written out directly.  NumPy only."""
import numpy as np

import policy_reference as R
import ppo_reference as G

# the shapes of tests/test_zz_asym_critic_gpu.py: (O, hidden, act_dim, (offset, dim)) -- a window narrower and wider than the actor's
# input, an offset that is no multiple of 4, a dim that is no multiple of 16, a window that ends exactly at the row stride
SHAPES = ((3, (16,), 1, (1, 17)), (33, (64, 64), 12, (0, 118)), (260, (32, 48), 7, (260, 85)), (20, (16, 32, 240), 4, (3, 512 - 3)))


def row_width(obs_dim, window):
    """Columns of a row the two towers read: the farther end of the two windows."""
    return max(obs_dim, window[0] + window[1])


def make_net(rng, obs_dim, hidden, act_dim, window, sigma=0.3):
    """``(actor, log_std, critic)`` as ppo_reference.make_net draws them, the critic's first layer ``window[1]`` wide."""
    actor, log_std, _ = G.make_net(rng, obs_dim, hidden, act_dim, value=False, sigma=sigma)
    critic = R.random_layers(rng, R.tower_shapes(window[1], hidden, 1), "linear")
    return actor, log_std, critic


def views(batch, obs_dim, window):
    """``(actor's batch, critic's batch)``: the wide batch with the observations cut to each tower's columns."""
    rows = np.asarray(batch.observations)
    off, dim = window
    return batch._replace(observations=rows[:, :obs_dim]), batch._replace(observations=rows[:, off:off + dim])


def values(critic, batch, obs_dim, window):
    return G._tower(critic, views(batch, obs_dim, window)[1].observations, False)[1][:, 0]


def loss_and_grad(actor, log_std, critic, batch, obs_dim, window, out_tanh=False, clip_range=0.2, clip_range_vf=None, ent_coef=0.0,
                  vf_coef=0.5):
    """``(stats, grad)`` as ppo_reference.loss_and_grad returns them, for wide rows ``batch.observations [B, >= row_width]``."""
    a_batch, c_batch = views(batch, obs_dim, window)
    p_stats, p_grad = G.loss_and_grad(actor, log_std, None, a_batch, out_tanh, clip_range, None, ent_coef, vf_coef)
    # the value part: ppo_reference needs an actor on the same observations; a one-layer zero actor's own terms are dropped
    act_dim = len(log_std)
    dummy = [(np.zeros((act_dim, window[1])), np.zeros(act_dim))]
    v_stats, v_grad = G.loss_and_grad(dummy, log_std, critic, c_batch, False, clip_range, clip_range_vf, 0.0, vf_coef)
    n_critic = sum(np.asarray(W).size + np.asarray(b).size for W, b in critic)
    stats = dict(p_stats, value_loss=v_stats["value_loss"])
    stats["loss"] = p_stats["policy_loss"] + ent_coef * p_stats["entropy_loss"] + vf_coef * v_stats["value_loss"]
    return stats, np.concatenate([p_grad, v_grad[len(v_grad) - n_critic:]])


def make_batch(rng, actor, log_std, critic, obs_dim, window, out_tanh, B, clip_range=0.2, clip_range_vf=None, pad=0):
    """A wide batch by ppo_reference's recipe: rows of ``row_width + pad`` columns; ``old_values`` around the critic's values on ITS
    window, redrawn away from the value-clip boundary."""
    width = row_width(obs_dim, window) + pad
    narrow = G.make_batch(rng, actor, log_std, None, out_tanh, B, clip_range, None)
    rows = (rng.standard_normal((B, width)) * np.logspace(-2, 1, width)).astype(np.float32)
    rows[:, :obs_dim] = narrow.observations
    wide = narrow._replace(observations=rows, returns=rng.standard_normal(B).astype(np.float32))
    v = values(critic, wide, obs_dim, window)
    old_v = (v + 0.3 * rng.standard_normal(B)).astype(np.float32)
    for _ in range(100):
        if not clip_range_vf:
            break
        bad = np.abs(np.abs(v - old_v.astype(np.float64)) - clip_range_vf) < G.BAND
        if not bad.any():
            break
        old_v[bad] = (v[bad] + 0.3 * rng.standard_normal(int(bad.sum()))).astype(np.float32)
    return wide._replace(old_values=old_v)
