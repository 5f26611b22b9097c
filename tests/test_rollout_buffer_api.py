"""The rollout buffer without a GPU: the float64 checker of tests/rollout_buffer_reference.py against hand-worked cases, the host-only
part of the C ABI (qg_rollout_* validate before the device check, no CPU backend) and DeviceRolloutBuffer's tensor checks."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import rollout_buffer_reference as R

from quadruped_gym_amd import _abi
from quadruped_gym_amd import rollout as RB

QG_ERR_ARG, QG_ERR_DEVICE = -1, -2


# -- the checker against hand-worked cases --------------------------------------------------------------------------------------------
def _gae(r, v, d, lv, gamma, lam):
    a, ret = R.gae(np.array(r, np.float64).reshape(-1, 1), np.array(v, np.float64).reshape(-1, 1), np.array(d).reshape(-1, 1),
                   np.array([lv], np.float64), gamma, lam)
    return a[:, 0], ret[:, 0]


def test_two_steps_one_env_without_a_done():
    # delta1 = 2 + 0.5 * 4 - 3 = 1; A1 = 1; delta0 = 1 + 0.5 * 3 - 2 = 0.5; A0 = 0.5 + 0.5 * 0.5 * 1 = 0.75
    a, ret = _gae([1.0, 2.0], [2.0, 3.0], [0, 0], 4.0, 0.5, 0.5)
    assert np.array_equal(a, [0.75, 1.0]) and np.array_equal(ret, [2.75, 4.0])


def test_nothing_flows_across_a_done_at_step_0():
    # the done stored with step 0 ends the episode there: delta0 = 1 - 2 = -1 and A1 does not enter A0
    a, ret = _gae([1.0, 2.0], [2.0, 3.0], [1, 0], 4.0, 0.5, 0.5)
    assert np.array_equal(a, [-1.0, 1.0]) and np.array_equal(ret, [1.0, 4.0])


def test_a_done_at_the_last_step_ignores_last_values():
    a, ret = _gae([1.0, 2.0], [2.0, 3.0], [0, 1], 1e9, 0.5, 0.5)
    # delta1 = 2 - 3 = -1; delta0 = 0.5 as before; A0 = 0.5 + 0.25 * -1 = 0.25
    assert np.array_equal(a, [0.25, -1.0]) and np.array_equal(ret, [2.25, 2.0])


def test_lambda_0_gives_the_one_step_delta():
    a, _ = _gae([1.0, 2.0, -1.0], [2.0, 3.0, 0.5], [0, 0, 0], 4.0, 0.5, 0.0)
    assert np.array_equal(a, [1.0 + 1.5 - 2.0, 2.0 + 0.25 - 3.0, -1.0 + 2.0 - 0.5])


def test_lambda_1_gamma_1_gives_the_undiscounted_sum_minus_the_value():
    r, v, lv = [1.0, 2.0, -1.0], [2.0, 3.0, 0.5], 4.0
    a, ret = _gae(r, v, [0, 0, 0], lv, 1.0, 1.0)
    assert np.array_equal(a, [1.0 + 2.0 - 1.0 + 4.0 - 2.0, 2.0 - 1.0 + 4.0 - 3.0, -1.0 + 4.0 - 0.5])
    assert np.array_equal(ret, [6.0, 5.0, 3.0])


def test_checker_add_bootstrap_episodes_partial_fill_and_gather():
    b = R.RolloutBuffer(2, 3, 1, 1, gamma=0.5, gae_lambda=1.0)
    b.begin(np.array([[10.0], [20.0]]))
    one = np.ones((2, 1))
    b.add(11 * one, one, [0.1, 0.2], [1.0, 2.0], [1.0, 2.0], [0, 1], trunc_value=[0.0, 8.0])
    b.add(12 * one, 2 * one, [0.3, 0.4], [3.0, 4.0], [3.0, 4.0], [1, 0], episode_reward=[30.0, 40.0])
    assert b.pos == 2 and np.array_equal(b.rewards[:2], [[1.0, 6.0], [3.0, 4.0]])            # 2 + 0.5 * 8
    assert np.array_equal(b.obs[:, 0, 0], [10.0, 11.0, 12.0, 0.0])
    # env 0: one episode of two steps with return 1 + 30; env 1: one of one step with return 2 (the stored 6 is not what is logged)
    assert b.episode_stats(clear=False) == (33.0, 3, 2)
    assert b.cur_return[1] == 40.0 and b.cur_length[1] == 1
    b.compute(np.array([100.0, 5.0]))
    # env 0: done at t = 1: A1 = 3 - 3 = 0, A0 = 1 + 0.5 * 3 - 1 + 0.5 * 0 = 1.5; env 1: A1 = 4 + 2.5 - 4 = 2.5, A0 = 6 - 2 = 4 (done at 0)
    assert np.array_equal(b.advantages[:2], [[1.5, 4.0], [0.0, 2.5]]) and np.array_equal(b.advantages[2], [0.0, 0.0])
    g = b.gather([3, -1, 0, 4])
    assert b.bad_index == 2
    assert np.array_equal(g["advantages"], [2.5, 0.0, 1.5, 0.0]) and np.array_equal(g["observations"][:, 0], [11.0, 0.0, 10.0, 0.0])
    b.add(13 * one, one, [0, 0], [0, 0], [0, 0], [0, 0])
    b.add(14 * one, one, [0, 0], [0, 0], [0, 0], [0, 0])
    assert b.pos == 3 and b.overflow == 1 and b.obs[3, 0, 0] == 13.0
    b.begin()
    assert b.pos == 0 and b.obs[0, 0, 0] == 13.0
    assert b.episode_stats() == (33.0, 3, 2) and b.episode_stats() == (0.0, 0, 0) and b.cur_length[1] == 2


def test_a_float32_loop_stays_inside_the_bound():
    """The bound of the GPU test, on the CPU: a NumPy float32 loop in the header's order against the float64 checker."""
    worst = 0.0
    for K, n, _, _ in R.SHAPES:
        for gamma, lam in R.GAE_PARAMS:
            for case in R.GAE_CASES:
                r, v, d, lv = R.gae_inputs(case, K, n)
                a64, r64 = R.gae(r.astype(np.float64), v.astype(np.float64), d, lv.astype(np.float64), gamma, lam)
                a32, r32 = R.gae(r, v, d, lv, gamma, lam)
                worst = max(worst, max(np.abs(a32 - a64).max(), np.abs(r32 - r64).max()) / R.gae_bound(r, v, a64, gamma, lam))
    assert 0.0 < worst < 0.5


# -- description and storage validation -----------------------------------------------------------------------------------------------
def _storage(**over):
    # addresses are never dereferenced on the host: any aligned non-NULL value passes the checks
    f = dict(obs=0x1000, actions=0x2000, log_prob=0x3000, values=0x4000, rewards=0x5000, advantages=0x6000, returns=0x7000, dones=0x8001)
    f.update(over)
    return _abi.QgRolloutStorage.make(**f)


BAD_DESC = {
    "n_envs 0": dict(n_envs=0), "n_steps 0": dict(n_steps=0), "obs_dim 0": dict(obs_dim=0), "obs_dim 513": dict(obs_dim=513),
    "act_dim 0": dict(act_dim=0), "act_dim 17": dict(act_dim=17), "gamma negative": dict(gamma=-0.1), "gamma above 1": dict(gamma=1.01),
    "gamma nan": dict(gamma=float("nan")), "lambda negative": dict(gae_lambda=-1e-9), "lambda above 1": dict(gae_lambda=2.0),
    "lambda inf": dict(gae_lambda=float("inf")), "too many rows": dict(n_envs=1 << 20, n_steps=2048), "struct_size": dict(struct_size=36),
}


@pytest.mark.parametrize("case", list(BAD_DESC))
def test_create_rejects_bad_descriptions(case):
    lib = _abi.load_library()
    args = dict(n_envs=64, n_steps=8, obs_dim=33, act_dim=12)
    args.update({k: v for k, v in BAD_DESC[case].items() if k != "struct_size"})
    d = _abi.QgRolloutDesc.make(**args)
    assert d.struct_size == 40
    if "struct_size" in BAD_DESC[case]:
        d.struct_size = BAD_DESC[case]["struct_size"]
    s, h = _storage(), C.c_void_p()
    assert lib.qg_rollout_create(0, C.byref(d), C.byref(s), C.byref(h)) == QG_ERR_ARG and not h.value
    assert len(lib.qg_last_error()) > 10


BAD_STORAGE = [(name, 0) for name in ("obs", "actions", "log_prob", "values", "rewards", "advantages", "returns", "dones")] + \
              [(name, 0x1002) for name in ("obs", "actions", "log_prob", "values", "rewards", "advantages", "returns")]


@pytest.mark.parametrize("name,value", BAD_STORAGE)
def test_create_rejects_null_and_misaligned_storage(name, value):
    lib = _abi.load_library()
    d, s, h = _abi.QgRolloutDesc.make(64, 8, 33, 12), _storage(**{name: value}), C.c_void_p()
    assert lib.qg_rollout_create(0, C.byref(d), C.byref(s), C.byref(h)) == QG_ERR_ARG and not h.value
    assert name.encode() in lib.qg_last_error()


def test_wrong_struct_size_is_refused_in_each_struct():
    lib = _abi.load_library()
    d, h = _abi.QgRolloutDesc.make(64, 8, 33, 12), C.c_void_p()
    s = _storage()
    assert s.struct_size == 72
    s.struct_size = 64
    assert lib.qg_rollout_create(0, C.byref(d), C.byref(s), C.byref(h)) == QG_ERR_ARG
    assert b"qg_rollout_storage.struct_size" in lib.qg_last_error()
    step = _abi.QgRolloutStep.make()
    assert step.struct_size == 88
    step.struct_size = 80
    assert lib.qg_rollout_add_device(None, C.byref(step), None) == QG_ERR_ARG
    assert b"qg_rollout_step.struct_size" in lib.qg_last_error()
    batch = _abi.QgRolloutBatch.make()
    assert batch.struct_size == 56
    batch.struct_size = 0
    assert lib.qg_rollout_gather_device(None, None, 4, C.byref(batch), None) == QG_ERR_ARG
    assert b"qg_rollout_batch.struct_size" in lib.qg_last_error()
    assert C.sizeof(_abi.QgRolloutInfo) == 24


def test_null_arguments_and_empty_batches_are_refused():
    lib = _abi.load_library()
    d, s, h = _abi.QgRolloutDesc.make(64, 8, 33, 12), _storage(), C.c_void_p()
    assert lib.qg_rollout_create(0, None, C.byref(s), C.byref(h)) == QG_ERR_ARG
    assert lib.qg_rollout_create(0, C.byref(d), None, C.byref(h)) == QG_ERR_ARG
    assert lib.qg_rollout_create(0, C.byref(d), C.byref(s), None) == QG_ERR_ARG
    batch = _abi.QgRolloutBatch.make()
    for B in (0, -1):
        assert lib.qg_rollout_gather_device(None, None, B, C.byref(batch), None) == QG_ERR_ARG
        assert b"at least one row" in lib.qg_last_error()
    assert lib.qg_rollout_gather_device(None, None, 4, None, None) == QG_ERR_ARG
    assert lib.qg_rollout_gather_device(None, None, 4, C.byref(batch), None) == QG_ERR_ARG
    assert lib.qg_rollout_begin_device(None, None, 1, None) == QG_ERR_ARG
    assert lib.qg_rollout_add_device(None, None, None) == QG_ERR_ARG
    assert lib.qg_rollout_add_device(None, C.byref(_abi.QgRolloutStep.make()), None) == QG_ERR_ARG
    assert lib.qg_rollout_compute_device(None, None, None) == QG_ERR_ARG
    assert lib.qg_rollout_get_info(None, None) == QG_ERR_ARG
    assert lib.qg_rollout_episode_stats(None, None, None, None, 0) == QG_ERR_ARG
    assert lib.qg_rollout_destroy(None) == 0
    assert (_abi.ROLLOUT_DONE_U8, _abi.ROLLOUT_DONE_F32) == (_abi.NORM_DONE_U8, _abi.NORM_DONE_F32)


@pytest.mark.skipif(torch.cuda.is_available(), reason="this check is for hosts without a GPU")
def test_a_valid_description_needs_a_device():
    lib = _abi.load_library()
    d, s, h = _abi.QgRolloutDesc.make(4096, 2048, 260, 12), _storage(), C.c_void_p()
    assert lib.qg_rollout_create(0, C.byref(d), C.byref(s), C.byref(h)) == QG_ERR_DEVICE and not h.value
    assert b"no CPU backend" in lib.qg_last_error() or b"hip" in lib.qg_last_error().lower()


# -- DeviceRolloutBuffer's tensor checks raise before any library call -----------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the tensors were checked")


def _hostless(n=8, K=4, D=6, A=3):
    """A DeviceRolloutBuffer without a handle (there is no device here): only its checks can run."""
    b = RB.DeviceRolloutBuffer.__new__(RB.DeviceRolloutBuffer)
    b._lib, b._h = _NoLibrary(), None
    b.num_envs, b.n_steps, b.obs_dim, b.act_dim, b.device = n, K, D, A, 0
    b._count, b._batch = 0, {}
    return b


def _fake(shape, dtype=torch.float32, strides=None):
    """A stand-in with a tensor's metadata that claims to be on the device."""
    t = torch.zeros(shape, dtype=dtype)
    return types.SimpleNamespace(is_cuda=True, device=types.SimpleNamespace(index=0), shape=t.shape, dtype=dtype, dim=t.dim,
                                 stride=(lambda i=None, s=strides or t.stride(): s if i is None else s[i]),
                                 is_contiguous=lambda: strides is None, data_ptr=lambda: 0)


def test_tensor_checks_raise_value_error_before_any_library_call():
    b = _hostless()
    cpu = torch.zeros
    good = dict(next_obs=_fake((8, 6)), actions=_fake((8, 3)), log_prob=_fake((8,)), value=_fake((8,)), reward=_fake((8,)),
                done=_fake((8,), torch.uint8))
    with pytest.raises(ValueError, match="cuda:0"):
        b.begin(cpu((8, 6)))
    with pytest.raises(ValueError, match="cuda:0"):
        b.add(**dict(good, next_obs=cpu((8, 6))))
    with pytest.raises(ValueError, match="cuda:0"):
        b.add(**dict(good, reward=cpu(8)))
    with pytest.raises(ValueError, match="cuda:0"):
        b.add_packed(cpu((8, 8)), good["actions"], good["log_prob"], good["value"])
    with pytest.raises(ValueError, match="cuda:0"):
        b.compute_returns_and_advantage(cpu(8))
    with pytest.raises(ValueError, match="cuda:0"):
        b.sample(torch.zeros(4, dtype=torch.int64))

    with pytest.raises(ValueError, match=r"\(8, 6\)"):
        b.begin(_fake((8, 5)))
    with pytest.raises(ValueError, match="stride"):
        b.begin(_fake((8, 6), strides=(4, 1)))
    with pytest.raises(ValueError, match="next_obs"):
        b.add(**dict(good, next_obs=_fake((7, 6))))
    with pytest.raises(ValueError, match="actions"):
        b.add(**dict(good, actions=_fake((8, 4))))
    with pytest.raises(ValueError, match="actions"):
        b.add(**dict(good, actions=_fake((8, 3), strides=(6, 2))))
    with pytest.raises(ValueError, match="log_prob"):
        b.add(**dict(good, log_prob=_fake((8,), torch.float64)))
    with pytest.raises(ValueError, match="value"):
        b.add(**dict(good, value=_fake((8, 1))))
    with pytest.raises(ValueError, match="reward"):
        b.add(**dict(good, reward=_fake((7,))))
    with pytest.raises(ValueError, match="done"):
        b.add(**dict(good, done=_fake((8,), torch.int32)))
    with pytest.raises(ValueError, match="trunc_value"):
        b.add(**dict(good, trunc_value=_fake((8,), torch.float16)))
    with pytest.raises(ValueError, match="episode_reward"):
        b.add(**dict(good, episode_reward=_fake((9,))))
    with pytest.raises(ValueError, match=r"\(8, 8\)"):
        b.add_packed(_fake((8, 7)), good["actions"], good["log_prob"], good["value"])
    with pytest.raises(ValueError, match="last_values"):
        b.compute_returns_and_advantage(_fake((8, 1)))
    with pytest.raises(ValueError, match="int64"):
        b.sample(_fake((4,), torch.int32))
    with pytest.raises(ValueError, match="int64"):
        b.sample(_fake((0,), torch.int64))
    out = RB.RolloutBufferSamples(_fake((4, 6)), _fake((4, 3)), _fake((4,)), _fake((5,)), None, None)
    with pytest.raises(ValueError, match="old_log_prob"):
        b.sample(_fake((4,), torch.int64), out=out)
    with pytest.raises(ValueError, match="batch_size"):
        next(b.get(0))
    assert b._count == 0
