"""``ContactSensor`` -- foot-contact sensing on the device (``qg_contact_*`` in ``include/quadgym.h``): the ground reaction force of
every body, the feet's position and velocity, contact flags and gait timers of the robots of a ``BatchedSim``, in one launch that only
reads the simulator's state.  The forces are those the NEXT substep would apply at the state as it stands in memory."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import FOOT_DIM, NBODY, NFOOT, QgContactDesc, check
from ._handle import Handle
from .task_layers import _TaskLayer, _mask_ptr


class ContactSensor(_TaskLayer):
    """Bound to ``sim`` (its ``Handle`` child, so it is destroyed before it).  A foot is in contact where the vertical ground force
    on it exceeds ``force_threshold`` (N)."""

    _destroy = "qg_contact_destroy"
    _abi_prefix = "qg_contact"
    FOOT_COLUMNS = _abi.FOOT_COLUMNS
    FOOT_BODIES = _abi.FOOT_BODIES

    def __init__(self, sim, force_threshold: float = 0.0):
        force_threshold = float(force_threshold)
        if not np.isfinite(force_threshold) or force_threshold < 0.0:
            raise ValueError(f"force_threshold must be finite and >= 0, got {force_threshold}")
        super().__init__(sim.device, parent=sim)
        self.num_envs = sim.n
        self.force_threshold = force_threshold
        self._create("qg_contact_create", sim._h, C.byref(QgContactDesc.make(force_threshold)))

    def _check_outputs(self, body_force, feet):
        """The optional outputs of a read (``read`` and ``GaitReward.step``): contiguous float32 ``[N, 13, 3]`` and ``[N, 4, 12]`` on
        this device, ``feet`` at a 16-byte boundary.  None passes; nothing is allocated."""
        import torch
        if body_force is not None:
            self._check_tensor(body_force, (self.num_envs, NBODY, 3), torch.float32, "body_force")
        if feet is not None:
            self._check_tensor(feet, (self.num_envs, NFOOT, FOOT_DIM), torch.float32, "feet")
            if feet.data_ptr() % 16:
                raise ValueError("feet: the rows are written with 16-byte stores; the tensor must be 16-byte aligned")

    def read(self, done=None, advance: bool = True, body_force=None, feet=None, stream=None):
        """One launch on ``stream`` (torch's current stream by default): ``(body_force [N, 13, 3], feet [N, 4, 12])`` float32 CUDA
        tensors, allocated unless passed.  ``advance=True`` moves the gait timers on by one env-step; ``done`` (uint8, bool or
        float32 ``[N]``, e.g. the step's) restarts the timers of the envs it names.  ``advance=False`` writes no timer and shows no
        event.  A bad argument raises ``ValueError`` before any launch."""
        import torch
        n = self.num_envs
        dev = self._torch_device()
        self._check_outputs(body_force, feet)
        dp, kind, stride = self._done_arg(done)
        if body_force is None:
            body_force = torch.empty((n, NBODY, 3), device=dev, dtype=torch.float32)
        if feet is None:
            feet = torch.empty((n, NFOOT, FOOT_DIM), device=dev, dtype=torch.float32)
        check(self._lib.qg_contact_read_device(self._h, dp, kind, stride, 1 if advance else 0, body_force.data_ptr(), feet.data_ptr(),
                                               self._stream_ptr(stream)), "qg_contact_read_device")
        return body_force, feet

    def read_host(self):
        """``(body_force [N, 13, 3], feet [N, 4, 12])`` as NumPy arrays: synchronous, the timers do not advance."""
        force = np.empty((self.num_envs, NBODY, 3), np.float32)
        feet = np.empty((self.num_envs, NFOOT, FOOT_DIM), np.float32)
        check(self._lib.qg_contact_read(self._h, force.ctypes.data, feet.ctypes.data), "qg_contact_read")
        return force, feet

    def reset(self, mask=None):
        """The next advancing read starts an episode for the envs of ``mask`` (all, when None)."""
        mask, mp = _mask_ptr(mask, self.num_envs)
        check(self._lib.qg_contact_reset(self._h, mp), "qg_contact_reset")
