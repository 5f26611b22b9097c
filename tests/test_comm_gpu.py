"""The native RCCL exchange (qg_comm_*) with a 1-rank communicator: the C loop must produce exactly what stepping
through qg_step_device_packed produces, and the gathered buffer must equal the packed one.  (Several ranks cannot be
exercised on a one-GPU box; the ordering logic is the same, the peers are not.)"""
import ctypes as C

import numpy as np
import pytest

from quadruped_gym_amd import _abi

pytestmark = pytest.mark.gpu


def test_native_rollout_matches_plain_stepping():
    import torch
    from quadruped_gym_amd._abi import check
    from quadruped_gym_amd.sim import BatchedSim
    lib = _abi.load_library()
    n, steps = 300, 7
    task = _abi.default_task()
    task.auto_reset = 1
    a_sim, b_sim = BatchedSim(n, task=task), BatchedSim(n, task=task)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    pool = [torch.rand((n, 12), generator=gen, device=dev) * 2 - 1 for _ in range(4)]
    # reference: plain stepping
    ref = torch.empty((n, 35), device=dev)
    refs = []
    for k in range(steps):
        b_sim.step_device_packed(pool[k % 4], ref)
        torch.cuda.synchronize()
        refs.append(ref.cpu().numpy().copy())
    # native loop
    uid = (C.c_uint8 * 128)()
    check(lib.qg_comm_unique_id(uid), "qg_comm_unique_id")
    comm = C.c_void_p()
    check(lib.qg_comm_create(a_sim._h, 0, 1, uid, C.byref(comm)), "qg_comm_create")
    packed = [torch.zeros((n, 35), device=dev) for _ in range(2)]
    gathered = [torch.zeros((1, n, 35), device=dev) for _ in range(2)]
    a_arr = (C.c_void_p * 4)(*[p.data_ptr() for p in pool])
    p_arr = (C.c_void_p * 2)(packed[0].data_ptr(), packed[1].data_ptr())
    g_arr = (C.c_void_p * 2)(gathered[0].data_ptr(), gathered[1].data_ptr())
    check(lib.qg_comm_rollout(comm, a_arr, 4, p_arr, g_arr, steps, 0), "qg_comm_rollout")
    check(lib.qg_comm_synchronize(comm), "qg_comm_synchronize")
    last, prev = (steps - 1) & 1, (steps - 2) & 1
    assert np.array_equal(gathered[last][0].cpu().numpy(), refs[-1])
    assert np.array_equal(gathered[prev][0].cpu().numpy(), refs[-2])
    assert np.array_equal(packed[last].cpu().numpy(), refs[-1])
    assert np.array_equal(a_sim.get_state()[0], b_sim.get_state()[0])
    # a second call continues the double-buffer protocol where the first one stopped
    check(lib.qg_comm_rollout(comm, a_arr, 4, p_arr, g_arr, 2, 0), "qg_comm_rollout")
    check(lib.qg_comm_synchronize(comm), "qg_comm_synchronize")
    for k in range(2):                                   # the call restarts at k = 0: pool[0], pool[1] into buffers 0, 1
        b_sim.step_device_packed(pool[k], ref)
    torch.cuda.synchronize()
    want = ref.cpu().numpy().tobytes()                   # bit for bit
    assert packed[1].cpu().numpy().tobytes() == want
    assert gathered[1][0].cpu().numpy().tobytes() == want
    assert a_sim.get_state()[0].tobytes() == b_sim.get_state()[0].tobytes()
    lib.qg_comm_destroy(comm)
    a_sim.close(); b_sim.close()
