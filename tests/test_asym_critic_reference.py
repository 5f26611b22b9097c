"""The asymmetric reference (tests/asym_critic_reference.py) against torch float64 autograd of the loss written out directly; the
arithmetic of FusedMlpPolicy.param_layout for asymmetric shapes; and the refusals of qg_policy_param_count_asym / qg_policy_create_asym
that precede the device check."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import asym_critic_reference as A

from quadruped_gym_amd import _abi
from quadruped_gym_amd.policy import FusedMlpPolicy

QG_ERR_ARG = -1


def _torch_loss(actor, log_std, critic, batch, obs_dim, window, out_tanh, c, cv, ent_coef, vf_coef):
    """SB3 2.x PPO.train's loss of one minibatch, the critic on its own columns; returns (loss, leaves in the canonical order)."""
    f64 = torch.float64
    leaf = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=f64, requires_grad=True)
    a_l, c_l, ls = [(leaf(W), leaf(b)) for W, b in actor], [(leaf(W), leaf(b)) for W, b in critic], leaf(log_std)
    rows = torch.tensor(np.asarray(batch.observations, np.float64))

    def tower(layers, x, last_tanh):
        for k, (W, b) in enumerate(layers):
            x = x @ W.T + b
            if k < len(layers) - 1 or last_tanh:
                x = torch.tanh(x)
        return x
    mean = tower(a_l, rows[:, :obs_dim], out_tanh)
    v = tower(c_l, rows[:, window[0]:window[0] + window[1]], False)[:, 0]
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    z = (t(batch.actions) - mean) / torch.exp(ls)
    logp = (-0.5 * z * z - ls - 0.5 * math.log(2 * math.pi)).sum(-1)
    r = torch.exp(logp - t(batch.old_log_prob))
    adv = t(batch.advantages)
    policy_loss = -torch.min(adv * r, adv * torch.clamp(r, 1 - c, 1 + c)).mean()
    vp = v if not cv else t(batch.old_values) + torch.clamp(v - t(batch.old_values), -cv, cv)
    value_loss = ((t(batch.returns) - vp) ** 2).mean()
    entropy_loss = -(0.5 + 0.5 * math.log(2 * math.pi) + ls).sum()
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    leaves = [p for Wb in a_l for p in Wb] + [ls] + [p for Wb in c_l for p in Wb]
    return loss, policy_loss, value_loss, leaves


@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "%d-%s-%d-%s" % (s[0], "x".join(map(str, s[1])), s[2], "+".join(map(str, s[3]))))
@pytest.mark.parametrize("cv", [None, 0.2])
def test_composed_gradient_is_autograds(shape, cv):
    O, hidden, act, window = shape
    rng = np.random.default_rng(O + 7 * len(hidden))
    out_tanh = O == 33
    actor, log_std, critic = A.make_net(rng, O, hidden, act, window)
    batch = A.make_batch(rng, actor, log_std, critic, O, window, out_tanh, 37, clip_range_vf=cv, pad=2)
    assert batch.observations.shape == (37, A.row_width(O, window) + 2)
    stats, grad = A.loss_and_grad(actor, log_std, critic, batch, O, window, out_tanh, 0.2, cv, 0.01, 0.5)
    loss, policy_loss, value_loss, leaves = _torch_loss(actor, log_std, critic, batch, O, window, out_tanh, 0.2, cv, 0.01, 0.5)
    loss.backward()
    want = np.concatenate([p.grad.numpy().ravel() for p in leaves])
    layout = FusedMlpPolicy.param_layout(O, hidden, act, True, critic_obs_dim=window[1])
    assert grad.shape == want.shape == (sum(int(np.prod(s)) for _, s in layout.values()),)
    scale = np.abs(want).max()
    assert np.abs(grad - want).max() <= 1e-12 * scale and scale > 1e-6
    lo = layout["critic.0.weight"][0]
    assert np.abs(want[lo:]).max() > 1e-8 and np.abs(want[:lo]).max() > 1e-8        # both towers carry gradient
    for got, ref in ((stats["loss"], loss), (stats["policy_loss"], policy_loss), (stats["value_loss"], value_loss)):
        assert abs(got - ref.item()) <= 1e-12 * max(1.0, abs(ref.item()))


def test_param_layout_of_asymmetric_shapes():
    lib = _abi.load_library()
    for O, hidden, act, (off, dim) in A.SHAPES:
        layout = FusedMlpPolicy.param_layout(O, hidden, act, True, critic_obs_dim=dim)
        sym = FusedMlpPolicy.param_layout(O, hidden, act, True)
        assert list(layout) == list(sym)
        end = 0
        for name, (at, shape) in layout.items():             # contiguous, in order
            assert at == end, name
            end += int(np.prod(shape))
        assert layout["actor.0.weight"] == sym["actor.0.weight"] == (0, (hidden[0], O)) and layout["log_std"] == sym["log_std"]
        assert layout["critic.0.weight"] == (sym["critic.0.weight"][0], (hidden[0], dim))
        assert end - sum(int(np.prod(s)) for _, s in sym.values()) == hidden[0] * (dim - O)
        desc = _abi.QgPolicyDesc.make(O, hidden, act, False, True)
        assert lib.qg_policy_param_count_asym(C.byref(desc), dim) == end
        assert lib.qg_policy_param_count_asym(C.byref(desc), O) == lib.qg_policy_param_count(C.byref(desc))
    assert FusedMlpPolicy.param_layout(33, (64,), 12, True, critic_obs_dim=None) == FusedMlpPolicy.param_layout(33, (64,), 12, True)
    assert FusedMlpPolicy.param_layout(33, (64,), 12, False, critic_obs_dim=85) == FusedMlpPolicy.param_layout(33, (64,), 12, False)


def test_refusals_precede_the_device_check():
    lib = _abi.load_library()
    good = _abi.QgPolicyDesc.make(33, (64, 64), 12, False, True)
    no_value = _abi.QgPolicyDesc.make(33, (64, 64), 12, False, False)
    bad_desc = _abi.QgPolicyDesc.make(33, (60,), 12, False, True)

    def create(desc, off, dim):
        h = C.c_void_p()
        rc = lib.qg_policy_create_asym(0, C.byref(desc), off, dim, C.byref(h))
        assert not h.value
        return rc, lib.qg_last_error().decode()
    cases = ((no_value, 0, 85, "has_value"), (good, 0, 0, "critic_obs_dim 0 outside 1 .. 512"), (good, 0, 513, "critic_obs_dim 513 outside 1 .. 512"),
             (good, 0, -1, "critic_obs_dim -1 outside 1 .. 512"), (good, 428, 85, "offset + dim = 513"), (good, -1, 85, "critic_obs_offset -1"),
             (good, 2 ** 31 - 1, 512, "critic_obs_offset 2147483647"), (bad_desc, 0, 85, "hidden[0] = 60"))
    for desc, off, dim, words in cases:
        rc, msg = create(desc, off, dim)
        assert rc == QG_ERR_ARG and words in msg, (off, dim, rc, msg)
        if off == 0:
            assert lib.qg_policy_param_count_asym(C.byref(desc), dim) == QG_ERR_ARG and words in lib.qg_last_error().decode()
    assert lib.qg_policy_create_asym(0, C.byref(good), 33, 85, None) == QG_ERR_ARG
    assert lib.qg_policy_param_count_asym(None, 85) == QG_ERR_ARG
    off, dim = C.c_int32(), C.c_int32()
    assert lib.qg_policy_critic_window(None, C.byref(off), C.byref(dim)) == QG_ERR_ARG
    # the widest window passes the validation: the count is the arithmetic's
    assert lib.qg_policy_param_count_asym(C.byref(good), 512) == lib.qg_policy_param_count(C.byref(good)) + 64 * (512 - 33)
    # Python: an asymmetric policy without a critic tower, and SB3's loader, are refused
    with pytest.raises(ValueError, match="value=False"):
        FusedMlpPolicy(33, (64,), 12, value=False, critic_obs=(33, 85))
    p = object.__new__(FusedMlpPolicy)
    p.out_tanh, p.asymmetric = False, True
    with pytest.raises(ValueError, match="asymmetric"):
        p.load_sb3_state_dict({})
