"""``DeviceVecEnvWrapper`` -- what the VecEnv wrappers around a device-side layer share (``DeviceVecNormalize``,
``DevicePerturbedVecEnv``): the wrapped env and the pass-through to it, the buffers of a ``step_tensor`` call by name, the upload
of the NumPy cold path, the finished envs whose info holds a terminal observation, and checkpoint / resume / close over the layer."""
from __future__ import annotations

import numpy as np

STEP_BUFFERS = ("obs", "reward", "done", "components", "terminal_obs")      # the walking envs' step_tensor, behind `actions`


class DeviceVecEnvWrapper:
    """``venv`` is a ``BatchedEnvBase``; ``layer`` the ``Handle`` whose launches follow (or precede) the env's on one stream.  A
    subclass names the layer's key of the snapshot dict in ``_snapshot_key`` and gives its state with ``_layer_state()`` /
    ``_load_layer_state(state)``.  Every attribute this class and the subclass do not define passes through to the wrapped env."""

    _snapshot_key = ""

    def __init__(self, venv, layer):
        self.venv = venv
        self._layer = layer
        self._packed = venv.packed_step                     # the plain env steps into packed [N, obs_dim + 2] rows

    def __getattr__(self, name):                            # only reached for what the classes do not define
        if name == "venv":                                  # (before __init__ has set it: no recursion)
            raise AttributeError(name)
        return getattr(self.venv, name)

    @staticmethod
    def _step_buffers(args, kwargs):
        """The buffers of ``step_tensor(actions, *args, **kwargs)`` by name, however the caller passed them."""
        bound = dict(zip(STEP_BUFFERS, args))
        bound.update({k: v for k, v in kwargs.items() if k in STEP_BUFFERS})
        return bound

    # -- NumPy cold path --------------------------------------------------------------------
    def _upload(self, array, dtype=np.float32):
        import torch
        return torch.from_numpy(np.ascontiguousarray(array, dtype=dtype)).to(self._layer._torch_device())

    @staticmethod
    def _finished_with_terminal(done, infos):
        """``[(i, infos[i])]`` of the finished envs whose info holds a terminal observation."""
        rows = [(int(i), infos[int(i)]) for i in np.nonzero(done)[0]]
        return [(i, info) for i, info in rows if isinstance(info, dict) and info.get("terminal_observation") is not None]

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    # -- checkpoint / resume ----------------------------------------------------------------
    def _layer_state(self):
        raise NotImplementedError

    def _load_layer_state(self, state):
        raise NotImplementedError

    def snapshot(self):
        """The wrapped env's snapshot with the layer's state beside it."""
        return {"env": self.venv.snapshot(), self._snapshot_key: self._layer_state()}

    def restore(self, snap):
        self.venv.restore(snap["env"])
        self._load_layer_state(snap[self._snapshot_key])

    def close(self):
        self._layer.close()
        self.venv.close()
