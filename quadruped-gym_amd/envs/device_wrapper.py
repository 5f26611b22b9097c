"""``DeviceVecEnvWrapper`` -- what the VecEnv wrappers around a device-side layer share (``DeviceVecNormalize``,
``DevicePerturbedVecEnv``, ``DeviceGaitRewardVecEnv``, ``DeviceGaitScheduleVecEnv``, ``DevicePrivilegedVecEnv``,
``DeviceCommandCurriculumVecEnv``): the wrapped env and the pass-through to it, the
buffers of a ``step_tensor`` call by name, the upload of the NumPy cold path, the finished envs whose info holds a terminal
observation, checkpoint / resume / close over the layer, and the walk along a stack's ``.venv`` chain by which a wrapper refuses, at
construction, an order of the stack that cannot work.

The orders that work, inside to outside: ``DevicePerturbedVecEnv`` next to the env (never around ``DevicePrivilegedVecEnv``: its
noise belongs on the actor's columns); ``DeviceGaitRewardVecEnv`` anywhere, but with ``gate_on_command=True`` inside any
``DeviceVecNormalize`` that normalises observations (the gate reads the command in m/s); ``DeviceGaitScheduleVecEnv`` around the walking
envs only (the plain env's packed rows have no command and no room for the clock), outside ``DevicePerturbedVecEnv`` (the clock is no
sensor), on either side of ``DeviceGaitRewardVecEnv``, inside ``DevicePrivilegedVecEnv`` (the actor's window must hold the clock) and,
with ``gate_on_command=True``, inside a normaliser of observations; ``DeviceVecNormalize`` outside
``DevicePrivilegedVecEnv`` around the walking envs, and inside it around the plain env, whose packed step keeps the wide rows apart;
``DeviceCommandCurriculumVecEnv`` around the walking envs only, built with ``random_controls=False``, and anywhere in the stack: it
touches no row, reward or component, so it goes on either side of ``DevicePerturbedVecEnv``, ``DeviceGaitRewardVecEnv``,
``DeviceGaitScheduleVecEnv``, ``DevicePrivilegedVecEnv`` and ``DeviceVecNormalize``.  Its criteria name columns of the layers INSIDE it,
so criteria on gait or schedule terms put it outside those wrappers; the gates of ``gate_on_command=True`` read the command that was
in force during the step, wherever the curriculum stands.  ``tests/wrapper_stacks.py`` lists the orders the suite steps: outside the
perturbation and inside the privileged wrapper, outside the gait and schedule wrappers and inside both."""
from __future__ import annotations

import numpy as np

STEP_BUFFERS = ("obs", "reward", "done", "components", "terminal_obs")      # the walking envs' step_tensor, behind `actions`


def stack_layers(venv):
    """The wrappers of the stack ``venv``, outermost first, along the ``.venv`` chain; the env itself is not among them."""
    while isinstance(venv, DeviceVecEnvWrapper):
        yield venv
        venv = venv.venv


def stack_layer(venv, key):
    """The outermost wrapper of the stack ``venv`` whose snapshot key is ``key`` (``"privileged"``, ``"normalizer"`` ...), or None."""
    return next((layer for layer in stack_layers(venv) if layer._snapshot_key == key), None)


def base_env(venv):
    """The env at the bottom of the stack ``venv``."""
    while isinstance(venv, DeviceVecEnvWrapper):
        venv = venv.venv
    return venv


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
