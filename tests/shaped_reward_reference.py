"""What the NumPy definitions of the shaped-reward layers share (tests/gait_reward_reference.py, tests/gait_schedule_reference.py): the
tail of `evaluate` behind a layer's unweighted terms -- weigh, zero the finished envs, sum in ascending order, add onto the reward, put
the base columns in front -- and the three tolerance functions over a layer's error budget.  A layer passes its own TERMS, BUDGET_TERM
and BUDGET_SUM_ULPS.  No GPU, no torch."""
import numpy as np


def weight_vector(weights, terms, dtype=np.float64):
    """[len(terms)] in the order of `terms`, as the float32 values the C ABI takes."""
    return np.array([np.float32(weights.get(name, 0.0)) for name in terms], np.float32).astype(dtype)


def tail(terms, weights, names, done=None, reward=None, base=None, dtype=np.float64):
    """The dict (components [n, NT], shaped [n], reward_out [n], wide [n, C0 + NT]) of the unweighted `terms` [n, NT]: every operation
    in `dtype`, the sum in ascending order, a finished env's components zero and its reward passed through."""
    T = dtype
    n, nt = terms.shape
    comps = (weight_vector(weights, names, T)[None] * terms).astype(T)
    finished = np.zeros(n, bool) if done is None else np.asarray(done) != 0
    comps[finished] = 0
    shaped = comps[:, 0].copy()
    for k in range(1, nt):                                        # ascending k
        shaped = (shaped + comps[:, k]).astype(T)
    if reward is None:
        out = shaped.copy()
    else:
        rew = np.asarray(reward, np.float32).astype(T)
        out = np.where(finished, rew, (rew + shaped).astype(T))
    wide = comps if base is None else np.concatenate([np.asarray(base, np.float32).astype(T), comps], axis=1)
    return dict(components=comps, shaped=shaped, reward_out=out, wide=wide)


def term_tolerance(terms64, names, budget_term, margin=1.0):
    """[n, NT]: margin x (atol + rtol |t64|) per unweighted term."""
    t = np.abs(np.asarray(terms64, np.float64))
    return margin * np.stack([budget_term[name][0] + budget_term[name][1] * t[:, k] for k, name in enumerate(names)], axis=1)


def component_tolerance(ref, weights, names, budget_term, margin=1.0):
    """[n, NT]: the terms' bounds times |w_k|, and the one rounding of f32(w_k x term_k)."""
    w = np.abs(weight_vector(weights, names))
    return w[None] * term_tolerance(ref["terms"], names, budget_term, margin) + margin * 2.0 ** -24 * np.abs(ref["components"])


def reward_tolerance(ref, weights, names, budget_term, sum_ulps, reward=None, margin=1.0):
    """[n]: the components' bounds summed, and `sum_ulps` roundings of half an ulp of the magnitudes added."""
    size = np.abs(ref["components"]).sum(1) + (0.0 if reward is None else np.abs(np.asarray(reward, np.float64)))
    return component_tolerance(ref, weights, names, budget_term, margin).sum(1) + margin * sum_ulps * 2.0 ** -24 * size
