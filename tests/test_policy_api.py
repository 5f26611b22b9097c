"""The fused MLP policy without a GPU: the float64 checker of tests/policy_reference.py against torch, the host-only part of the C
ABI (qg_policy_param_count, argument validation before the device check, no CPU backend), the parameter loaders' flat order, and
the two censuses of tests/policy_reference.py's SHAPE_TABLE: the branch conditions it reaches, and the kernel instantiations."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import policy_reference as R

from quadruped_gym_amd import _abi
from quadruped_gym_amd import policy as P

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


# ---- the shape table of tests/test_policy_shapes_gpu.py ----------------------------------------------------------------------------
def _ids(desc):
    return "%d-%s-%d" % (desc[0], "-".join(str(h) for h in desc[1]), desc[2])


# Every branch condition of the forward pass (policy_reference.conditions) in every launch shape <waves, blocks> where it can occur.
# It cannot occur: <4,1> holds one block per wave (no single / partial / uneven) and its 32-block round covers obs_dim <= 512 in one;
# on one wave no wave is idle and none differs from another; <1,16> advances by single input blocks (nq >= kq = 1, no partly live
# half-chunk).  Written out, so that a row deleted from the table fails here.
_EDGES = {"obs:no-padding", "obs<4", "obs=512", "act:partial-group", "act<4", "lds1:hidden2", "lds0:hidden1"}
REQUIRED = {
    (4, 1): _EDGES | {"hidden:idle", "hidden:full",
                      "chunk:nq<kq", "chunk:second-half-off", "chunk:multiple", "chunk:second-half-partial"},
    (4, 4): _EDGES | {"hidden:idle", "hidden:single", "hidden:partial", "hidden:full", "hidden:uneven",
                      "chunk:nq<kq", "chunk:second-half-off", "chunk:multiple", "chunk:second-half-partial", "chunk:rounds>1"},
    (1, 4): _EDGES | {"hidden:single", "hidden:partial", "hidden:full",
                      "chunk:nq<kq", "chunk:second-half-off", "chunk:multiple", "chunk:second-half-partial", "chunk:rounds>1"},
    (1, 16): _EDGES | {"hidden:single", "hidden:partial", "hidden:full",
                       "chunk:second-half-off", "chunk:multiple", "chunk:rounds>1"},
}


def _census(table):
    return set().union(*(R.conditions(desc, waves) for desc in table for waves in (1, 4)))


def test_shape_table_reaches_every_branch_condition():
    required = {(w, b, name) for (w, b), names in REQUIRED.items() for name in names}
    reached = _census(R.SHAPE_TABLE)
    assert required - reached == set(), "branch conditions no row of SHAPE_TABLE reaches"
    assert reached - required == set(), "conditions() names something the census does not require"


def test_conditions_of_known_layers():
    """conditions() against block counts worked out by hand: 80 / 144 / 208 / 240 wide on four waves are 2/1/1/1, 3/2/2/2, 4/3/3/3 and
    4/4/4/3 blocks per wave."""
    def hidden(desc, waves):
        return {name for _, _, name in R.conditions(desc, waves) if name.startswith("hidden:")}
    assert hidden((1, (80,), 1), 4) == {"hidden:single", "hidden:partial", "hidden:uneven"}
    assert hidden((33, (144,), 12), 4) == {"hidden:partial", "hidden:uneven"}
    assert hidden((260, (208,), 12), 4) == {"hidden:partial", "hidden:full", "hidden:uneven"}
    assert hidden((129, (240, 96, 176), 15), 4) == {"hidden:partial", "hidden:full", "hidden:uneven", "hidden:single"}
    assert hidden((512, (256, 256, 256), 16), 4) == {"hidden:full"} == hidden((512, (256, 256, 256), 16), 1)
    assert hidden((65, (16, 16, 16), 2), 4) == {"hidden:idle", "hidden:full"} and hidden((65, (16, 16, 16), 2), 1) == {"hidden:single"}
    assert hidden((20, (16, 32, 240), 4), 1) == {"hidden:single", "hidden:partial"}
    assert {b for _, b, _ in R.conditions((1, (80,), 1), 1)} == {16} and {b for _, b, _ in R.conditions((1, (16,), 1), 4)} == {1}
    # 65 inputs are five blocks: on <1,4> (rounds of 8) the second half-chunk is partly live; on <4,1> (rounds of 32) it is off
    assert (1, 4, "chunk:second-half-partial") in R.conditions((65, (16, 16, 16), 2), 1)
    assert (4, 1, "chunk:second-half-off") in R.conditions((65, (16, 16, 16), 2), 4)


def test_launch_sites_equal_what_the_table_launches():
    """Every instantiation of qg_policy_forward_kernel the library can launch is one the table reaches (each row runs at one and at
    four waves in tests/test_policy_shapes_gpu.py), and the other way round: a fifth launch site fails here until a row reaches it."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quadruped-gym_amd", "csrc", "qg_policy.hip")).read()
    sites = {(int(w), int(b)) for w, b in re.findall(r"launch_policy<\s*(\d+)\s*,\s*(\d+)\s*>\s*\(", src)}
    assert sites == {(4, 1), (4, 4), (1, 4), (1, 16)}
    kernels = {(int(w), int(b)) for w, b in re.findall(r"qg_policy_forward_kernel<\s*(\w+)\s*,\s*(\w+)\s*>", src) if w.isdigit()}
    assert kernels == set()                            # the kernel is launched through launch_policy alone
    reached = {R.launch_shape(hidden, n, towers, 1024, force) for _, hidden, _ in R.SHAPE_TABLE for n in (83, 16 * 1024)
               for towers in (1, 2) for force in (1, 4)}
    assert reached == sites == set(REQUIRED)
    # the rule itself, on the numbers of an MI355X: 1024 SIMDs
    assert R.launch_shape((64, 64), 4096, 1, 1024) == (4, 1) and R.launch_shape((64, 64), 16384, 1, 1024) == (1, 4)
    assert R.launch_shape((64, 64), 16369, 1, 1024) == (1, 4) and R.launch_shape((64, 64), 16368, 1, 1024) == (4, 1)
    assert R.launch_shape((64, 64), 8192, 2, 1024) == (1, 4) and R.launch_shape((64, 64), 8176, 2, 1024) == (4, 1)
    assert R.launch_shape((64, 80), 1 << 20, 2, 1024) == (4, 4) and R.launch_shape((256,), 1, 1, 1024, force_waves=1) == (1, 16)


@pytest.mark.parametrize("value", [False, True])
@pytest.mark.parametrize("desc", R.SHAPE_TABLE, ids=_ids)
def test_param_count_over_the_table(desc, value):
    obs_dim, hidden, act_dim = desc
    d = _abi.QgPolicyDesc.make(obs_dim, hidden, act_dim, False, value)
    want = act_dim                                     # log_std; then (in + 1) x out per layer of each tower
    for out_dim in (act_dim, 1)[:2 if value else 1]:
        dims = (obs_dim,) + hidden + (out_dim,)
        want += sum((dims[k] + 1) * dims[k + 1] for k in range(len(dims) - 1))
    assert _abi.load_library().qg_policy_param_count(C.byref(d)) == R.param_count(obs_dim, hidden, act_dim, value) == want


@pytest.mark.parametrize("desc", R.SHAPE_TABLE, ids=_ids)
def test_checker_equals_torch_float64_over_the_table(desc):
    obs_dim, hidden, act_dim = desc
    rng = np.random.default_rng(1)
    out_tanh = bool(R.SHAPE_TABLE.index(desc) % 2)
    actor = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, act_dim), "linear")
    critic = R.random_layers(rng, R.tower_shapes(obs_dim, hidden, 1), "sb3", head_gain=1.0)
    obs = (rng.standard_normal((37, obs_dim)) * np.logspace(-2, 1, obs_dim)).astype(np.float32)
    mean, _, _, value = R.forward(actor, np.zeros(act_dim), obs, critic=critic, out_tanh=out_tanh)
    with torch.no_grad():
        x = torch.from_numpy(obs).double()
        t_mean = _sequential(actor, out_tanh, torch.float64)(x).numpy()
        t_value = _sequential(critic, False, torch.float64)(x).numpy()[:, 0]
    assert mean.shape == (37, act_dim) and value.shape == (37,)
    assert np.abs(mean - t_mean).max() <= 1e-12
    assert np.abs(value - t_value).max() <= 1e-12 * max(1.0, np.abs(t_value).max())


@pytest.mark.parametrize("desc", [(512, (256, 256, 256), 16), (1, (16,), 1)], ids=_ids)
def test_descriptions_at_the_limits_are_accepted(desc):
    obs_dim, hidden, act_dim = desc
    lib = _abi.load_library()
    for value in (False, True):
        d = _abi.QgPolicyDesc.make(obs_dim, hidden, act_dim, True, value)
        assert lib.qg_policy_param_count(C.byref(d)) == R.param_count(obs_dim, hidden, act_dim, value) > 0


def test_launch_shape_needs_a_handle():
    lib = _abi.load_library()
    waves, blocks = C.c_int32(-7), C.c_int32(-7)
    assert lib.qg_policy_launch_shape(None, 83, 0, C.byref(waves), C.byref(blocks)) == QG_ERR_ARG
    assert (waves.value, blocks.value) == (-7, -7)
