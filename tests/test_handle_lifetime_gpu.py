"""Every handle gives back the device memory it took: the destroy functions free what the handle's allocation owner recorded
(csrc/qg_host.h, QgDevMem) instead of a list of pointers kept by hand, so a leak would be an allocation made outside the owner.

One round creates a simulator of 70 envs (one full wave of the one-link-per-lane kernel and a ragged tail of 6) with a walking layer
and a partially observable layer of window 3 on it, a 33-64-64-12 policy with a critic and a 70 x 33 normaliser, steps each once and
destroys them -- once in each legal order (the layers before their simulator; the policy and the normaliser before or after).
After an untimed round that loads the code objects, free device memory after round 3 must not be below free memory after round 1.

Baseline: the same rounds on the parent commit (hand-kept free lists) on an MI355X read 308 382 007 296 bytes free after the warm-up
and after each of the three rounds: the parent drifts by 0 bytes, so no allowance is made.  (This code, same visit: 308 375 715 840
four times.)"""
import ctypes as C

import pytest
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd.normalize import RunningNormalizer
from quadruped_gym_amd.policy import FusedMlpPolicy
from quadruped_gym_amd.sim import BatchedSim

pytestmark = pytest.mark.gpu

N, WINDOW = 70, 3


def _one_pass(layers_first):
    """Create everything, step each handle once, destroy: the simulator's chain first (po, walk, sim) or last."""
    lib = _abi.load_library()
    dev = torch.device("cuda:0")
    f32 = dict(dtype=torch.float32, device=dev)
    acts = torch.rand((N, 12), **f32) * 2 - 1
    reward, done = torch.empty(N, **f32), torch.empty(N, dtype=torch.uint8, device=dev)

    sim = BatchedSim(N, device=0)
    packed = torch.empty((N, sim.obs_dim + 2), **f32)
    sim.step_device_packed(acts, packed)
    walk, po = C.c_void_p(), C.c_void_p()
    _abi.check(lib.qg_walk_create(sim._h, None, C.byref(walk)), "qg_walk_create")
    _abi.check(lib.qg_po_create(walk, WINDOW, C.byref(po)), "qg_po_create")
    obs33 = torch.empty((N, 33), **f32)
    _abi.check(lib.qg_walk_step_device(walk, acts.data_ptr(), obs33.data_ptr(), reward.data_ptr(), done.data_ptr(), None,
                                       sim._stream_ptr(None)), "qg_walk_step_device")
    assert lib.qg_po_obs_dim(po) == 26 * WINDOW
    stack = torch.empty((N, 26 * WINDOW), **f32)
    _abi.check(lib.qg_po_step_device(po, acts.data_ptr(), stack.data_ptr(), reward.data_ptr(), done.data_ptr(), None, None,
                                     sim._stream_ptr(None)), "qg_po_step_device")

    policy = FusedMlpPolicy(33, (64, 64), 12, value=True)
    policy.forward(obs33, torch.empty((N, 12), **f32), log_prob=torch.empty(N, **f32), value=torch.empty(N, **f32))
    norm = RunningNormalizer(N, 33)
    norm.step(obs33, reward, done)
    torch.cuda.synchronize()

    def chain():
        assert lib.qg_po_destroy(po) == 0 and lib.qg_walk_destroy(walk) == 0
        sim.close()

    def others():
        policy.close()
        norm.close()

    for destroy in ((chain, others) if layers_first else (others, chain)):
        destroy()


def rounds(count=4):
    """Free device memory (bytes) after each round; the first round is the warm-up that loads the code objects."""
    free = []
    for _ in range(count):
        _one_pass(True)
        _one_pass(False)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    return free


def test_handles_return_their_device_memory():
    free = rounds()
    print("free device memory after the warm-up and rounds 1..3:", free)
    assert free[3] >= free[1]


def test_failed_create_takes_no_device_memory():
    lib = _abi.load_library()
    good = FusedMlpPolicy(33, (64, 64), 12)            # the code object is loaded before the first reading
    good.close()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    desc = _abi.QgPolicyDesc.make(33, (24,), 12, False, True)          # 24 is not a multiple of 16
    h = C.c_void_p()
    assert lib.qg_policy_create(0, C.byref(desc), C.byref(h)) == -1 and not h.value          # QG_ERR_ARG
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == before
