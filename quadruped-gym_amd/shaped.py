"""What the shaped-reward layers share (``gait.py``: the gait terms; ``schedule.py``: the gait schedule) on the Python side of the tail
their launches end in (``csrc/qg_shaped_dev.h``): the weights by name, the one overlap a narrow block and the wide rows it is copied into
may have, the reward / component / command arguments of a ``step``, and what the two VecEnv wrappers do for ``gate_on_command``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import MONITOR_MAX_TERMS, check
from .envs.device_wrapper import stack_layers


def term_weights(weights, terms) -> list:
    """``[len(terms)]`` floats in the order of ``terms`` from ``{name: w}`` (missing names weigh 0) or None (all 0).  An unknown name or
    a non-finite weight raises ``ValueError``."""
    weights = dict(weights or {})
    unknown = sorted(set(weights) - set(terms))
    if unknown:
        raise ValueError(f"weights: unknown reward terms {unknown}: one of {', '.join(terms)}")
    out = [float(weights.get(name, 0.0)) for name in terms]
    for name, w in zip(terms, out):
        if not np.isfinite(w):
            raise ValueError(f"weights[{name!r}] must be finite, got {w}")
    return out


def _span(t, width, stride):
    lo = t.data_ptr()
    return lo, lo + 4 * ((t.shape[0] - 1) * stride + width)


def refuse_overlap(narrow, width, n_stride, wide, wide_width, w_stride, message):
    """``narrow`` (``[N, width]`` rows at ``n_stride``) is copied to the front of ``wide`` (``[N, wide_width]`` at ``w_stride``): it may
    be ``wide[:, :width]`` itself -- the same rows at the same stride, nothing is copied --, any other overlap of the two would let a
    lane read what another one writes: ``ValueError(message)``."""
    if not width or (narrow.data_ptr() == wide.data_ptr() and n_stride == w_stride):
        return
    (a0, a1), (b0, b1) = _span(narrow, width, n_stride), _span(wide, wide_width, w_stride)
    if a0 < b1 and b0 < a1:
        raise ValueError(message)


class ShapedReward:
    """Mixin of the ``Handle`` of a shaped-reward layer; the class names its terms in ``TERMS`` and its entry points' prefix in
    ``_abi_prefix``, the instance keeps ``weights`` (``{name: w}``)."""

    TERMS = ()

    def set_weights(self, weights):
        """New weights ``{name: w}`` for the launches that follow (missing names keep their weight); a captured graph keeps the
        weights it was captured with."""
        w, what = term_weights(dict(self.weights, **dict(weights)), self.TERMS), self._abi_prefix + "_set_weights"
        check(getattr(self._lib, what)(self._h, (C.c_float * len(w))(*w)), what)
        self.weights = dict(zip(self.TERMS, w))

    def _shaped_args(self, done, reward, reward_out, components, base_components, command, also=None):
        """The arguments every shaped launch takes, checked: ``(done3, rows11, components, reward_out)`` -- the done vector's
        ``(pointer, kind, stride)``, then ``(reward, stride, reward_out, stride, components, stride, base_components, stride, C0,
        command, stride)`` in the entry points' order, and the two outputs, allocated where the caller passed none.  The caller's
        tensors first, every one of them -- ``also()`` holds the checks of the layer's other tensors --; what is missing is allocated
        behind the checks."""
        import torch
        nt = len(self.TERMS)
        max_base = MONITOR_MAX_TERMS - nt
        done3 = self._done_arg(done)
        r_ptr, r_stride = None, 1
        if reward is not None:
            r_stride, r_ptr = self._check_vec(reward, (torch.float32,), "reward"), reward.data_ptr()
        o_stride = 1 if reward_out is None else self._check_vec(reward_out, (torch.float32,), "reward_out")
        b_ptr, b_stride, c0 = None, 0, 0
        if base_components is not None:
            if base_components.dim() != 2 or not 0 <= base_components.shape[1] <= max_base:
                raise ValueError(f"base_components: expected [N, C0] with C0 <= {max_base}, got {tuple(base_components.shape)}")
            c0 = int(base_components.shape[1])
            b_stride, b_ptr = self._check_rows(base_components, c0, "base_components"), base_components.data_ptr()
        c_stride = c0 + nt
        if components is not None:
            c_stride = self._check_rows(components, c0 + nt, "components")
            if c0:
                refuse_overlap(base_components, c0, b_stride, components, c0 + nt, c_stride,
                               "base_components and components overlap: allowed only where base_components is components[:, :C0]")
        m_ptr, m_stride = None, 2
        if command is not None:
            m_stride, m_ptr = self._check_rows(command, 2, "command"), command.data_ptr()
        if also is not None:
            also()
        if reward_out is None:
            reward_out = torch.empty(self.num_envs, device=self._torch_device(), dtype=torch.float32)
        if components is None:
            components = torch.empty((self.num_envs, c0 + nt), device=self._torch_device(), dtype=torch.float32)
        rows11 = (r_ptr, r_stride, reward_out.data_ptr(), o_stride, components.data_ptr(), c_stride, b_ptr, b_stride, c0, m_ptr, m_stride)
        return done3, rows11, components, reward_out


class CommandGated:
    """Mixin of the ``DeviceVecEnvWrapper`` of a shaped-reward layer: ``gate_on_command`` and the wrapper's scratch rows."""

    PO_COMMAND = 23                        # the command's vx, vy in a partially observable frame (po_walking_quad.py:48-56)

    @staticmethod
    def _check_gate(venv, gate_on_command, hint):
        """The two refusals of ``gate_on_command=True``, before any handle exists; ``hint`` names the order that works."""
        if gate_on_command and not hasattr(venv, "obs_window"):
            raise ValueError("gate_on_command: only the partially observable env's observation holds the command")
        if gate_on_command and any(layer._snapshot_key == "normalizer" and layer.normalizer.norm_obs for layer in stack_layers(venv)):
            raise ValueError("gate_on_command around a DeviceVecNormalize that normalises observations: the gate would compare normalised "
                             "command columns with min_command_speed in m/s; " + hint)

    def _command(self, obs):
        """The newest frame's (vx, vy) of the env's stacked observation, as a strided view."""
        if not self.gate_on_command:
            return None
        lo = (self.venv.obs_window - 1) * self.venv.FRAME + self.PO_COMMAND
        return obs[:, lo:lo + 2]

    def _rows(self, name, width):
        """The wrapper's own ``[N, width]`` rows kept in the attribute ``name`` (None until the first call that needs them)."""
        import torch
        buf = getattr(self, name)
        if buf is None or buf.shape[1] != width:
            buf = torch.empty((self.num_envs, width), device=self._layer._torch_device(), dtype=torch.float32)
            setattr(self, name, buf)
        return buf
