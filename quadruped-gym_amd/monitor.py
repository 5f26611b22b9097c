"""``RewardMonitor`` -- the reference's ``RewardCallback`` (``train_quadruped.py:60-110``) for a training loop that never leaves the
GPU (``qg_monitor_*`` of ``include/quadgym.h``, ``csrc/qg_monitor.hip``): at every env-step the mean of every reward term over the
envs, the reward's mean and standard deviation and the number of finished envs go into a ring on the device, and every term is summed
over the episodes -- what ``ep_rew_mean`` is for the whole reward, split by term.

One ``record`` is two small launches of hand-written gfx950 code on the caller's stream.  The ring's cursor lives in device memory, so
a hipGraph of ONE closed-loop step fills K rows when it is replayed K times.  PyTorch is plumbing only: it owns the ring and the
stream.  There is no CPU path.  Outputs for non-finite inputs are unspecified (train the walking envs with ``nan_direction=False``).
"""
from __future__ import annotations

import csv
import ctypes as C

import numpy as np

from ._abi import MONITOR_MAX_TERMS, check
from ._handle import Handle

# the ring's three columns behind the terms' and the reward's means
TAIL = ("std", "dones")


def real_time_columns(keys):
    """The header of the reference's ``rewards_continuous.csv`` (``RewardCallback.real_time_column``)."""
    return ["Training Steps"] + list(keys) + ["Reward"]


class RewardMonitor(Handle):
    """``log``: the ring, a torch float64 ``[capacity, len(keys) + 3]`` this object owns -- per row the means of the terms in the order
    of ``keys``, the reward's mean, its population standard deviation and the number of envs that finished --, written only by the
    library's launches.  The semantics of every call are stated in ``include/quadgym.h``."""

    _destroy = "qg_monitor_destroy"

    def __init__(self, num_envs: int, keys, capacity: int = 4096, device: int = 0):
        super().__init__(device)
        import torch
        self.num_envs, self.keys, self.capacity = int(num_envs), [str(k) for k in keys], int(capacity)
        self.n_terms = len(self.keys)
        if self.num_envs < 1 or self.capacity < 1:
            raise ValueError("num_envs and capacity must be >= 1")
        if not 1 <= self.n_terms <= MONITOR_MAX_TERMS:
            raise ValueError(f"keys: 1 .. {MONITOR_MAX_TERMS} reward terms, got {self.n_terms}")
        if len(set(self.keys)) != self.n_terms or set(self.keys) & {"step", "reward", *TAIL}:
            raise ValueError(f"keys must be distinct and none of step, reward, {', '.join(TAIL)}: {self.keys}")
        self._create("qg_monitor_create", self.device, self.num_envs, self.n_terms, self.capacity)
        self.log = torch.zeros((self.capacity, self.n_terms + 3), device=self._torch_device(), dtype=torch.float64)

    @classmethod
    def for_env(cls, env, capacity: int = 4096):
        """A monitor of ``env``'s size, device and ``reward_keys``: any of the VecEnvs or a device-side wrapper around one."""
        return cls(env.num_envs, list(env.reward_keys), capacity=capacity, device=getattr(env, "device", 0))

    # -- device path ------------------------------------------------------------------------
    def record(self, components, reward, done=None, stream=None):
        """One env-step: ``components`` float32 ``[N, len(keys)]`` (strided rows allowed), ``reward`` float32 ``[N]`` at any positive
        stride, ``done`` uint8 / bool / float32 ``[N]`` or None (nobody finished)."""
        import torch
        c_stride = self._check_rows(components, self.n_terms, "components")
        r_stride = self._check_vec(reward, (torch.float32,), "reward")
        d_ptr, kind, d_stride = self._done_arg(done)
        check(self._lib.qg_monitor_record_device(self._h, components.data_ptr(), c_stride, reward.data_ptr(), r_stride, d_ptr, kind, d_stride,
                                                 self.log.data_ptr(), self._stream_ptr(stream)), "qg_monitor_record_device")

    # -- reading ----------------------------------------------------------------------------
    def _info(self, clear=False):
        totals = np.empty(self.n_terms + 1)
        rec, eps, ls = C.c_int64(), C.c_int64(), C.c_int64()
        check(self._lib.qg_monitor_get_info(self._h, C.byref(rec), C.byref(eps), C.byref(ls), totals.ctypes.data, int(bool(clear))),
              "qg_monitor_get_info")
        return int(rec.value), int(eps.value), int(ls.value), totals

    @property
    def records(self):
        """The device's cursor: the number of records since creation or the last ``reset(clear_log=True)`` (waits for the device)."""
        return self._info()[0]

    def rows(self):
        """The last ``min(records, capacity)`` rows in chronological order: ``{"step": int64[], <key>: f64[], "reward", "std",
        "dones"}`` (NumPy).  Waits for the device; not during a capture."""
        records = self._info()[0]
        k = min(records, self.capacity)
        steps = np.arange(records - k, records, dtype=np.int64)
        table = self.log.cpu().numpy()[steps % self.capacity]
        out = {"step": steps}
        for c, name in enumerate(self.keys + ["reward", *TAIL]):
            out[name] = table[:, c].copy()
        return out

    def to_csv(self, path):
        """``rows()`` in the reference's real-time format (``rewards_continuous.csv``: header ``Training Steps,<keys...>,Reward``), so
        that the reference's dashboard reads the file unchanged."""
        rows = self.rows()
        with open(path, "w", newline="") as fh:
            fh.write(",".join(real_time_columns(self.keys)) + "\n")
            writer = csv.writer(fh)
            for j, step in enumerate(rows["step"]):
                writer.writerow([int(step)] + [float(rows[k][j]) for k in self.keys] + [float(rows["reward"][j])])

    def episode_stats(self, clear=True):
        """Over the episodes finished since the last clear: their number ``episodes``, ``ep_len_mean``, ``ep_rew_mean`` and ``terms``,
        the mean episode sum of every key (the means are NaN while no episode has finished); the raw ``totals``, ``length_sum`` and
        ``records`` beside them.  Waits for the device.  ``clear`` keeps the running episodes."""
        records, n, length_sum, totals = self._info(clear)
        nan = float("nan")
        return {"episodes": n, "ep_len_mean": length_sum / n if n else nan, "ep_rew_mean": float(totals[-1]) / n if n else nan,
                "terms": {k: (float(totals[c]) / n if n else nan) for c, k in enumerate(self.keys)},
                "totals": totals, "length_sum": length_sum, "records": records}

    def reset(self, mask=None, clear_totals=False, clear_log=False):
        """Empties the running accumulators of the envs ``mask`` selects (a host array ``[N]``; None: every env), as after an env's
        ``reset()``.  ``clear_totals`` also forgets the finished episodes, ``clear_log`` the rows recorded so far."""
        ptr = None
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            if mask.shape != (self.num_envs,):
                raise ValueError(f"mask: expected shape ({self.num_envs},), got {mask.shape}")
            ptr = mask.ctypes.data
        check(self._lib.qg_monitor_reset(self._h, ptr, int(bool(clear_totals)), int(bool(clear_log))), "qg_monitor_reset")
        if clear_log:
            self.log.zero_()

    # -- state ------------------------------------------------------------------------------
    def state(self):
        """Everything a resumed run needs (NumPy; waits for the device): ``acc [N, len(keys) + 1]``, ``len [N]``, ``totals``,
        ``episodes``, ``length_sum``, ``records`` and the ring ``log``."""
        acc, length = np.empty((self.num_envs, self.n_terms + 1)), np.empty(self.num_envs, np.int32)
        totals = np.empty(self.n_terms + 1)
        eps, ls, rec = C.c_int64(), C.c_int64(), C.c_int64()
        check(self._lib.qg_monitor_get_state(self._h, acc.ctypes.data, length.ctypes.data, totals.ctypes.data, C.byref(eps), C.byref(ls),
                                             C.byref(rec)), "qg_monitor_get_state")
        return {"acc": acc, "len": length, "totals": totals, "episodes": int(eps.value), "length_sum": int(ls.value),
                "records": int(rec.value), "log": self.log.cpu().numpy()}

    def load_state(self, state):
        import torch
        acc = np.ascontiguousarray(state["acc"], dtype=np.float64)
        length = np.ascontiguousarray(state["len"], dtype=np.int32)
        totals = np.ascontiguousarray(state["totals"], dtype=np.float64)
        log = np.ascontiguousarray(state["log"], dtype=np.float64)
        if (acc.shape != (self.num_envs, self.n_terms + 1) or length.shape != (self.num_envs,) or totals.shape != (self.n_terms + 1,)
                or log.shape != tuple(self.log.shape)):
            raise ValueError(f"the state was taken from a monitor of another shape: acc {acc.shape}, len {length.shape}, "
                             f"totals {totals.shape}, log {log.shape}")
        check(self._lib.qg_monitor_set_state(self._h, acc.ctypes.data, length.ctypes.data, totals.ctypes.data, int(state["episodes"]),
                                             int(state["length_sum"]), int(state["records"])), "qg_monitor_set_state")
        self.log.copy_(torch.from_numpy(log))
