"""The fused MLP policy without a GPU: the float64 checker of tests/policy_reference.py against torch, the host-only part of the C
ABI (qg_policy_param_count, argument validation before the device check, no CPU backend) and the parameter loaders' flat order."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import policy_reference as R  # noqa: E402

from quadruped_gym_amd import _abi  # noqa: E402
from quadruped_gym_amd import policy as P  # noqa: E402

QG_ERR_ARG, QG_ERR_DEVICE = -1, -2


def _sequential(layers, out_tanh, dtype):
    mods = []
    for k, (W, b) in enumerate(layers):
        lin = torch.nn.Linear(W.shape[1], W.shape[0]).to(dtype)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W).to(dtype))
            lin.bias.copy_(torch.from_numpy(b).to(dtype))
        mods.append(lin)
        if k < len(layers) - 1 or out_tanh:
            mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods)


@pytest.mark.parametrize("shape", list(R.SHAPES))
@pytest.mark.parametrize("out_tanh", [False, True])
def test_checker_equals_torch_float64(shape, out_tanh):
    obs_dim, hidden, act_dim = R.SHAPES[shape]
    rng = np.random.default_rng(1)
    actor = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, act_dim), "linear")
    critic = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, 1), "sb3", head_gain=1.0)
    obs = (rng.standard_normal((37, obs_dim)) * np.logspace(-2, 1, obs_dim)).astype(np.float32)
    mean, _, _, value = R.forward(actor, np.zeros(act_dim), obs, critic=critic, out_tanh=out_tanh)
    with torch.no_grad():
        x = torch.from_numpy(obs).double()
        t_mean = _sequential(actor, out_tanh, torch.float64)(x).numpy()
        t_value = _sequential(critic, False, torch.float64)(x).numpy()[:, 0]
    assert np.abs(mean - t_mean).max() <= 1e-12
    assert np.abs(value - t_value).max() <= 1e-12 * max(1.0, np.abs(t_value).max())


def test_checker_log_prob_equals_torch_normal():
    rng = np.random.default_rng(2)
    obs_dim, hidden, act_dim = R.SHAPES["plain"]
    actor = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, act_dim), "sb3")
    log_std = rng.uniform(-1.5, 0.5, act_dim)
    obs = rng.standard_normal((50, obs_dim))
    eps = rng.standard_normal((50, act_dim))
    mean, action, log_prob, _ = R.forward(actor, log_std, obs, eps=eps)
    dist = torch.distributions.Normal(torch.from_numpy(mean), torch.from_numpy(np.exp(log_std)))
    want = dist.log_prob(torch.from_numpy(action)).sum(-1).numpy()
    assert np.abs(log_prob - want).max() <= 1e-9          # (a - mean) / std rebuilds eps to rounding only
    # eps = None: the density at the mean
    _, action0, lp0, _ = R.forward(actor, log_std, obs)
    assert np.array_equal(action0, mean)
    assert np.abs(lp0 - dist.log_prob(torch.from_numpy(mean)).sum(-1).numpy()).max() <= 1e-12


@pytest.mark.parametrize("shape", list(R.SHAPES))
@pytest.mark.parametrize("value", [False, True])
def test_param_count(shape, value):
    obs_dim, hidden, act_dim = R.SHAPES[shape]
    lib = _abi.load_library()
    d = _abi.QgPolicyDesc.make(obs_dim, hidden, act_dim, False, value)
    assert d.struct_size == 36
    assert lib.qg_policy_param_count(C.byref(d)) == R.param_count(obs_dim, hidden, act_dim, value)
    towers = [R.tower_shapes(obs_dim, hidden, act_dim)] + ([R.tower_shapes(obs_dim, hidden, 1)] if value else [])
    assert R.param_count(obs_dim, hidden, act_dim, value) == sum(o * i + o for t in towers for o, i in t) + act_dim


def _bad_descriptions():
    def desc(**kw):
        d = _abi.QgPolicyDesc.make(33, (64, 64), 12, False, True)
        for k, v in kw.items():
            if k == "hidden0":
                d.hidden[0] = v
            else:
                setattr(d, k, v)
        return d
    return {"struct_size": desc(struct_size=32), "width_not_multiple_of_16": desc(hidden0=40), "n_hidden_0": desc(n_hidden=0),
            "n_hidden_4": desc(n_hidden=4), "act_dim_17": desc(act_dim=17), "obs_dim_0": desc(obs_dim=0), "width_272": desc(hidden0=272),
            "obs_dim_513": desc(obs_dim=513), "out_tanh_2": desc(out_tanh=2)}


@pytest.mark.parametrize("case", list(_bad_descriptions()))
def test_create_rejects_bad_descriptions(case):
    """Validation comes before the device check: QG_ERR_ARG with or without a GPU."""
    lib = _abi.load_library()
    d = _bad_descriptions()[case]
    h = C.c_void_p()
    assert lib.qg_policy_create(0, C.byref(d), C.byref(h)) == QG_ERR_ARG and not h.value
    assert lib.qg_last_error()
    assert lib.qg_policy_param_count(C.byref(d)) == QG_ERR_ARG
    assert lib.qg_policy_create(0, None, C.byref(h)) == QG_ERR_ARG


def test_null_handles_are_refused():
    lib = _abi.load_library()
    buf = (C.c_float * 4)()
    assert lib.qg_policy_set_params(None, buf) == QG_ERR_ARG
    assert lib.qg_policy_get_params(None, buf) == QG_ERR_ARG
    assert lib.qg_policy_set_params_device(None, buf, None) == QG_ERR_ARG
    assert lib.qg_policy_forward_device(None, 1, buf, 33, None, buf, None, None, None) == QG_ERR_ARG
    assert lib.qg_policy_destroy(None) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="this check is for hosts without a GPU")
def test_no_cpu_backend():
    lib = _abi.load_library()
    d = _abi.QgPolicyDesc.make(33, (64, 64), 12, True, True)
    h = C.c_void_p()
    assert lib.qg_policy_create(0, C.byref(d), C.byref(h)) == QG_ERR_DEVICE and not h.value
    with pytest.raises(_abi.QuadGymError):
        P.FusedMlpPolicy(33, (64, 64), 12)


class _Recorder(P.FusedMlpPolicy):
    """The loaders without a device: records the flat vector set_params would upload."""

    def __init__(self, obs_dim, hidden, act_dim, out_tanh=False, value=True):
        self.obs_dim, self.act_dim, self.hidden = obs_dim, act_dim, tuple(hidden)
        self.out_tanh, self.has_value = out_tanh, value
        self.n_params = R.param_count(obs_dim, hidden, act_dim, value)
        self._h = None
        self.flat = None

    def set_params(self, flat):
        flat = np.asarray(flat)
        assert flat.dtype == np.float32 and flat.shape == (self.n_params,)
        self.flat = flat


@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_loaders_agree_on_the_flat_vector(shape):
    obs_dim, hidden, act_dim = R.SHAPES[shape]
    rng = np.random.default_rng(3)
    actor = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, act_dim), "sb3")
    critic = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, 1), "sb3", head_gain=1.0)
    log_std = rng.uniform(-1, 0, act_dim).astype(np.float32)
    want = R.flatten(actor, log_std, critic)

    sd = {"log_std": torch.from_numpy(log_std)}
    for tower, prefix, head in ((actor, "mlp_extractor.policy_net", "action_net"), (critic, "mlp_extractor.value_net", "value_net")):
        for k, (W, b) in enumerate(tower):
            name = f"{prefix}.{2 * k}" if k < len(tower) - 1 else head
            sd[f"{name}.weight"], sd[f"{name}.bias"] = torch.from_numpy(W), torch.from_numpy(b)
    a = _Recorder(obs_dim, hidden, act_dim)
    a.load_sb3_state_dict(sd)
    b = _Recorder(obs_dim, hidden, act_dim)
    b.load_module(_sequential(actor, False, torch.float32), _sequential(critic, False, torch.float32), log_std)
    c = _Recorder(obs_dim, hidden, act_dim)
    c.load_layers(actor, log_std, critic)
    assert np.array_equal(a.flat, want) and np.array_equal(b.flat, want) and np.array_equal(c.flat, want)
    # the flat order is the header's: first the actor's W[out][in] row-major, then its bias
    o, i = R.tower_shapes(obs_dim, hidden, act_dim)[0]
    assert np.array_equal(want[:o * i].reshape(o, i), actor[0][0]) and np.array_equal(want[o * i:o * i + o], actor[0][1])


def test_loaders_refuse_what_the_kernel_cannot_run():
    p = _Recorder(33, (64, 64), 12, out_tanh=False, value=False)
    relu = torch.nn.Sequential(torch.nn.Linear(33, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 12))
    with pytest.raises(ValueError):
        p.load_module(relu)
    tanh_out = torch.nn.Sequential(torch.nn.Linear(33, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, 12),
                                   torch.nn.Tanh())
    with pytest.raises(ValueError):
        p.load_module(tanh_out)                        # out_tanh is False
    with pytest.raises(ValueError):
        p.load_layers([(np.zeros((64, 33)), np.zeros(64))])      # too few layers
    assert math.isclose(0.5 * math.log(2 * math.pi), 0.91893853320467274178)
