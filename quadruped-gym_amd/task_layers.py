"""``WalkLayer`` and ``ObsPack`` -- Python handles of the two task layers of the C ABI (``qg_walk_*`` / ``qg_po_*`` in
``include/quadgym.h``): the walking task bound to a ``BatchedSim`` and the partially observable observation pack bound to a
``WalkLayer``.  Each is the ``Handle`` child of what it is bound to, so it is destroyed before it (``_handle.py``)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import NU, NWALKREWARD, QgWalkParams, check
from ._handle import Handle


def default_walk_params() -> QgWalkParams:
    p = QgWalkParams()
    check(_abi.load_library().qg_walk_default_params(C.byref(p)), "qg_walk_default_params")
    return p


def _mask_ptr(mask, n):
    if mask is None:
        return None, None
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    if mask.shape != (n,):
        raise ValueError(f"mask: expected shape ({n},), got {mask.shape}")
    return mask, mask.ctypes.data


class _TaskLayer(Handle):
    """What the two layers share: the snapshot blob (``<_abi_prefix>_state_bytes`` / ``_get_state`` / ``_set_state`` of the ABI), the
    host buffers of a step and the checks of the tensors of ``step_device``."""

    _abi_prefix = ""

    def state_bytes(self) -> int:
        what = self._abi_prefix + "_state_bytes"
        fn = getattr(self._lib, what)
        if isinstance(_abi.PROTOTYPES[what], tuple):        # the size is the result
            nbytes = int(fn(self._h))
            if nbytes <= 0:               # the C side reports errors as small negative numbers
                check(nbytes if nbytes < 0 else -1, what)
            return nbytes
        nbytes = C.c_int64()                                # the status is the result, the size comes through a pointer
        check(fn(self._h, C.byref(nbytes)), what)
        return int(nbytes.value)

    def state(self):
        """The layer's per-env state as one ``uint8`` blob; ``load_state(blob)`` on a layer of the same shape continues bit for bit."""
        blob = np.empty(self.state_bytes(), np.uint8)
        check(getattr(self._lib, self._abi_prefix + "_get_state")(self._h, blob.ctypes.data), self._abi_prefix + "_get_state")
        return blob

    def check_state(self, blob):
        """``blob`` as contiguous ``uint8``; raises ``ValueError`` unless it has the size of this layer's state.  Writes nothing."""
        blob, nbytes = np.ascontiguousarray(blob, dtype=np.uint8), self.state_bytes()
        if blob.size != nbytes:
            raise ValueError(f"the blob holds {blob.size} bytes, this layer's state {nbytes}: it was taken from another shape")
        return blob

    def load_state(self, blob):
        blob = self.check_state(blob)
        check(getattr(self._lib, self._abi_prefix + "_set_state")(self._h, blob.ctypes.data), self._abi_prefix + "_set_state")

    def _host_step_buffers(self, actions):
        n = self.num_envs
        a = np.ascontiguousarray(actions, dtype=np.float32)
        if a.shape != (n, NU):
            raise ValueError(f"actions must have shape ({n}, {NU})")
        return (a, np.empty((n, self.obs_dim), np.float32), np.empty(n, np.float32), np.empty(n, np.uint8),
                np.empty((n, NWALKREWARD), np.float32))

    def _check_step(self, actions, obs, reward, done, components, terminal_obs=None):
        """Every tensor on this device, contiguous, of exactly the shape and dtype the kernel writes: the C side takes bare pointers."""
        import torch
        n = self.num_envs
        self._check_tensor(actions, (n, NU), torch.float32, "actions")
        self._check_tensor(obs, (n, self.obs_dim), torch.float32, "obs")
        self._check_tensor(reward, (n,), torch.float32, "reward")
        self._check_tensor(done, (n,), torch.bool if done.dtype == torch.bool else torch.uint8, "done")     # both one byte
        if components is not None:
            self._check_tensor(components, (n, NWALKREWARD), torch.float32, "components")
        if terminal_obs is not None:
            self._check_tensor(terminal_obs, (n, self.obs_dim), torch.float32, "terminal_obs")


class WalkLayer(_TaskLayer):
    """The walking task (command, settling mask, control-signal estimator, 11-term reward, flip / time-limit terminations) on the
    robots of ``sim``; one per simulator."""

    _destroy = "qg_walk_destroy"
    _abi_prefix = "qg_walk"
    obs_dim = 33

    def __init__(self, sim, params: QgWalkParams | None = None):
        super().__init__(sim.device, parent=sim)
        self.num_envs = sim.n
        self.params = params if params is not None else default_walk_params()
        self._create("qg_walk_create", sim._h, C.byref(self.params))

    def reset(self, seed: int = 0, flags: int = 0, mask=None):
        mask, mp = _mask_ptr(mask, self.num_envs)
        check(self._lib.qg_walk_reset(self._h, mp, int(seed), int(flags)), "qg_walk_reset")

    def step(self, actions):
        """NumPy in and out: ``(obs [n,33], reward [n], done [n] uint8, components [n,11])``."""
        a, obs, rew, done, comps = self._host_step_buffers(actions)
        check(self._lib.qg_walk_step(self._h, a.ctypes.data, obs.ctypes.data, rew.ctypes.data, done.ctypes.data, comps.ctypes.data),
              "qg_walk_step")
        return obs, rew, done, comps

    def step_device(self, actions, obs, reward, done, components=None, stream=None):
        self._check_step(actions, obs, reward, done, components)
        check(self._lib.qg_walk_step_device(self._h, actions.data_ptr(), obs.data_ptr(), reward.data_ptr(), done.data_ptr(),
                                            components.data_ptr() if components is not None else None, self._stream_ptr(stream)),
              "qg_walk_step_device")

    def set_commands(self, velocity, heading):
        """``[n, 2]`` contiguous float32 each."""
        check(self._lib.qg_walk_set_commands(self._h, velocity.ctypes.data, heading.ctypes.data), "qg_walk_set_commands")

    def get_commands(self, velocity, heading):
        """Fills the two ``[n, 2]`` float32 arrays with the commands as they stand on the device."""
        check(self._lib.qg_walk_get_commands(self._h, velocity.ctypes.data, heading.ctypes.data), "qg_walk_get_commands")

    def set_command_sampler(self, sampler):
        check(self._lib.qg_walk_set_command_sampler(self._h, C.byref(sampler)), "qg_walk_set_command_sampler")

    def estimates(self):
        """``(frequency [n,12], amplitude [n,12], ideal [n,2])`` of the control-signal estimator."""
        f, a = np.empty((self.num_envs, 12), np.float32), np.empty((self.num_envs, 12), np.float32)
        ideal = np.empty((self.num_envs, 2), np.float32)
        check(self._lib.qg_walk_get_estimates(self._h, f.ctypes.data, a.ctypes.data, ideal.ctypes.data), "qg_walk_get_estimates")
        return f, a, ideal


class ObsPack(_TaskLayer):
    """The stack of the last ``obs_window`` 26-value frames per robot, on top of ``walk``."""

    _destroy = "qg_po_destroy"
    _abi_prefix = "qg_po"

    def __init__(self, walk: WalkLayer, obs_window: int = 1):
        super().__init__(walk.device, parent=walk)
        self.num_envs, self.obs_window = walk.num_envs, int(obs_window)
        self._create("qg_po_create", walk._h, self.obs_window)
        self.obs_dim = int(self._lib.qg_po_obs_dim(self._h))
        self._terminal = None             # scratch for the library's terminal stacks of step()

    def reset(self, seed: int = 0, flags: int = 0, mask=None):
        mask, mp = _mask_ptr(mask, self.num_envs)
        obs = np.empty((self.num_envs, self.obs_dim), np.float32)
        check(self._lib.qg_po_reset(self._h, mp, int(seed), int(flags), obs.ctypes.data), "qg_po_reset")
        return obs

    def step(self, actions):
        """NumPy in and out: ``(obs, reward, done, components, terminal)``; ``terminal`` (the stack each finished env ended with) is
        scratch the next ``step`` overwrites -- copy the rows to keep."""
        a, obs, rew, done, comps = self._host_step_buffers(actions)
        if self._terminal is None:
            self._terminal = np.empty((self.num_envs, self.obs_dim), np.float32)
        check(self._lib.qg_po_step(self._h, a.ctypes.data, obs.ctypes.data, rew.ctypes.data, done.ctypes.data, comps.ctypes.data,
                                   self._terminal.ctypes.data), "qg_po_step")
        return obs, rew, done, comps, self._terminal

    def step_device(self, actions, obs, reward, done, components=None, terminal_obs=None, stream=None):
        self._check_step(actions, obs, reward, done, components, terminal_obs)
        check(self._lib.qg_po_step_device(self._h, actions.data_ptr(), obs.data_ptr(), reward.data_ptr(), done.data_ptr(),
                                          components.data_ptr() if components is not None else None,
                                          terminal_obs.data_ptr() if terminal_obs is not None else None, self._stream_ptr(stream)),
              "qg_po_step_device")
