"""The running normaliser without a GPU: the float64 checker of tests/normalize_reference.py against itself, the host-only part of the
C ABI (qg_norm_create validates before the device check, no CPU backend) and RunningNormalizer's tensor checks."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import normalize_reference as R

from quadruped_gym_amd import _abi
from quadruped_gym_amd import normalize as N

QG_ERR_ARG, QG_ERR_DEVICE = -1, -2


# -- the checker against itself -------------------------------------------------------------------------------------------------------
def test_two_updates_give_the_statistics_of_the_concatenation():
    rng = np.random.default_rng(0)
    A, B = R.columns(rng, 83, 26, 0).astype(np.float64), R.columns(rng, 17, 26, 1).astype(np.float64)
    rms = R.RunningMeanStd((26,))
    rms.update(A)
    rms.update(B)
    both = np.concatenate([A, B])
    # the prior (mean 0, var 1) enters as 1e-4 pseudo-rows: the closed form of merging it with the 100 real ones
    n, c0 = both.shape[0], 1e-4
    tot = c0 + n
    mean = both.mean(0) * n / tot
    var = (c0 * 1.0 + n * both.var(0) + both.mean(0) ** 2 * c0 * n / tot) / tot
    assert rms.count == tot
    scale = np.abs(both).max(0)
    assert np.all(np.abs(rms.mean - mean) <= 1e-12 * scale)
    assert np.all(np.abs(rms.var - var) <= 1e-12 * var)


def test_fresh_statistics_and_identity_before_any_update():
    nz = R.Normalizer(4, 5)
    assert np.array_equal(nz.obs_rms.mean, np.zeros(5)) and np.array_equal(nz.obs_rms.var, np.ones(5)) and nz.obs_rms.count == 1e-4
    assert nz.ret_rms.mean == 0.0 and nz.ret_rms.var == 1.0 and nz.ret_rms.count == 1e-4
    nz.training = False
    x = np.linspace(-2, 2, 20, dtype=np.float32).reshape(4, 5)
    out, _ = nz.step(x)
    assert np.array_equal(nz.obs_rms.mean, np.zeros(5)) and np.array_equal(nz.obs_rms.var, np.ones(5))
    assert np.abs(out - x).max() <= 1e-7                   # / sqrt(1 + 1e-8)


def test_constant_column_normalises_to_zero():
    nz = R.Normalizer(64, 3)
    x = np.full((64, 3), 9.81, np.float32)
    for _ in range(50):
        out, _ = nz.step(x)
    assert np.abs(out).max() <= 1e-3                        # the 1e-4 pseudo-rows of the prior are all that is left
    rms = R.RunningMeanStd((3,))
    rms.mean[:], rms.var[:] = 9.81, 0.0
    assert np.array_equal(R.apply(np.float64(9.81) * np.ones((2, 3)), rms.mean, rms.var, 1e-8, 10.0), np.zeros((2, 3), np.float32))


def test_values_beyond_the_clip_come_out_exactly_at_the_clip():
    nz = R.Normalizer(8, 1, clip_obs=5.0, clip_reward=2.5)
    nz.training = False
    x = np.array([[-1e6], [-5.0001], [-5.0], [0.0], [4.9999], [5.0001], [7.0], [1e30]], np.float32)
    out, rew = nz.step(x, reward=x[:, 0])
    assert np.array_equal(out[[0, 1, 5, 6, 7], 0], np.float32([-5, -5, 5, 5, 5]))
    assert np.abs(out[[3, 4], 0]).max() < 5.0
    assert np.array_equal(rew[[0, 1, 5, 6, 7]], np.float32([-2.5, -2.5, 2.5, 2.5, 2.5]))


def test_returns_are_zeroed_after_the_done_not_before_the_reward_is_added():
    nz = R.Normalizer(2, 1, gamma=0.5)
    obs = np.zeros((2, 1), np.float32)
    nz.step(obs, np.float32([1.0, 1.0]), np.array([0, 0]))
    assert np.array_equal(nz.returns, [1.0, 1.0])
    nz.step(obs, np.float32([2.0, 2.0]), np.array([1, 0]))
    # the statistic saw 0.5 * 1 + 2 for both envs before env 0 was cleared
    assert np.array_equal(nz.returns, [0.0, 2.5])
    batch1, batch2 = np.array([1.0, 1.0]), np.array([2.5, 2.5])
    rms = R.RunningMeanStd(())
    rms.update(batch1)
    rms.update(batch2)
    assert nz.ret_rms.mean == rms.mean and nz.ret_rms.var == rms.var and nz.ret_rms.count == 1e-4 + 4
    nz.step(obs, np.float32([1.0, 1.0]), np.array([0, 0]))
    assert np.array_equal(nz.returns, [1.0, 2.25])
    # training off: nothing moves, a done included
    nz.training = False
    before = nz.state()
    nz.step(obs, np.float32([3.0, 3.0]), np.array([1, 1]))
    after = nz.state()
    assert all(np.array_equal(before[k], after[k]) for k in before)


# -- description validation -----------------------------------------------------------------------------------------------------------
BAD = {
    "obs_dim 0": dict(obs_dim=0), "obs_dim 513": dict(obs_dim=513), "n_envs 0": dict(n_envs=0), "negative epsilon": dict(epsilon=-1e-8),
    "clip_obs 0": dict(clip_obs=0.0), "clip_reward negative": dict(clip_reward=-1.0), "struct_size": dict(struct_size=52),
}


@pytest.mark.parametrize("case", list(BAD))
def test_create_rejects_bad_descriptions(case):
    lib = _abi.load_library()
    args = dict(obs_dim=33, n_envs=64)
    args.update({k: v for k, v in BAD[case].items() if k != "struct_size"})
    d = _abi.QgNormDesc.make(**args)
    assert d.struct_size == 56
    if "struct_size" in BAD[case]:
        d.struct_size = BAD[case]["struct_size"]
    h = C.c_void_p()
    assert lib.qg_norm_create(0, C.byref(d), C.byref(h)) == QG_ERR_ARG and not h.value
    assert len(lib.qg_last_error()) > 10


def test_null_arguments_are_refused():
    lib = _abi.load_library()
    h = C.c_void_p()
    assert lib.qg_norm_create(0, None, C.byref(h)) == QG_ERR_ARG
    assert lib.qg_norm_step_device(None, 1, None, 1, None, 1, None, 1, None, 1, None, 0, 1, 1, None) == QG_ERR_ARG
    assert lib.qg_norm_update_obs_device(None, 1, None, 1, None) == QG_ERR_ARG
    assert lib.qg_norm_apply_obs_device(None, 1, None, 1, None, 1, None) == QG_ERR_ARG
    assert lib.qg_norm_reset_returns_device(None, None) == QG_ERR_ARG
    assert lib.qg_norm_get_state(None, None, None, None, None, None, None, None) == QG_ERR_ARG
    assert lib.qg_norm_set_state(None, None, None, 1.0, 0.0, 1.0, 1.0, None) == QG_ERR_ARG
    assert lib.qg_norm_destroy(None) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="this check is for hosts without a GPU")
def test_a_valid_description_needs_a_device():
    lib = _abi.load_library()
    d = _abi.QgNormDesc.make(260, 4096)
    h = C.c_void_p()
    assert lib.qg_norm_create(0, C.byref(d), C.byref(h)) == QG_ERR_DEVICE and not h.value
    with pytest.raises(_abi.QuadGymError):
        N.RunningNormalizer(64, 33)


# -- RunningNormalizer's tensor checks raise before any library call -------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the tensors were checked")


def _hostless(n=8, D=6):
    """A RunningNormalizer without a handle (there is no device here): only its checks can run."""
    nz = N.RunningNormalizer.__new__(N.RunningNormalizer)
    nz._lib, nz._h = _NoLibrary(), None
    nz.num_envs, nz.obs_dim, nz.device, nz.training = n, D, 0, True
    return nz


def test_tensor_checks_raise_value_error_before_any_library_call():
    nz = _hostless()
    cpu = torch.zeros((8, 6))
    with pytest.raises(ValueError, match="cuda:0"):
        nz.step(cpu)
    with pytest.raises(ValueError, match="cuda:0"):
        nz.update_obs(cpu)
    with pytest.raises(ValueError, match="cuda:0"):
        nz.normalize_obs(cpu)
    with pytest.raises(ValueError, match="cuda:0"):
        nz.step_packed(torch.zeros((8, 8)))

    # shape, dtype and stride checks need tensors that claim to be on the device: stand-ins with a tensor's metadata
    def fake(shape, dtype=torch.float32, strides=None):
        t = torch.zeros(shape, dtype=dtype)
        return types.SimpleNamespace(is_cuda=True, device=types.SimpleNamespace(index=0), shape=t.shape, dtype=dtype, dim=t.dim,
                                     stride=(lambda i=None, s=strides or t.stride(): s if i is None else s[i]),
                                     is_contiguous=lambda: strides is None, data_ptr=lambda: 0)
    with pytest.raises(ValueError, match=r"\(8, 6\)"):
        nz.step(fake((8, 5)))
    with pytest.raises(ValueError, match=r"\(8, 6\)"):
        nz.step(fake((7, 6)))
    with pytest.raises(ValueError, match="float32"):
        nz.step(fake((8, 6), torch.float64))
    with pytest.raises(ValueError, match="stride"):
        nz.step(fake((8, 6), strides=(4, 1)))
    with pytest.raises(ValueError, match="stride"):
        nz.normalize_obs(fake((8, 6), strides=(1, 8)))
    with pytest.raises(ValueError, match="obs_out"):
        nz.step(fake((8, 6)), obs_out=fake((8, 7)))
    with pytest.raises(ValueError, match="reward"):
        nz.step(fake((8, 6)), reward=fake((7,)))
    with pytest.raises(ValueError, match="done"):
        nz.step(fake((8, 6)), reward=fake((8,)), done=fake((8,), torch.int32))
    with pytest.raises(ValueError, match="need a reward"):
        nz.step(fake((8, 6)), done=fake((8,), torch.uint8))
    with pytest.raises(ValueError, match=r"\(8, 8\)"):
        nz.step_packed(fake((8, 7)))
    with pytest.raises(ValueError, match="another shape"):
        nz.load_state_dict({"obs_rms.mean": np.zeros(5), "obs_rms.var": np.ones(5), "returns": np.zeros(8)})
