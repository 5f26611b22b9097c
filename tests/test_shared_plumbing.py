"""What the device-side layers share, without a GPU: one pair of done constants under five names, one prototype table behind the
binding, one way to fill `struct_size`, one strided-rows check, the two forms of a state size, the shaped-reward layers' arguments, the
ledgers of what the layers' C and Python code share, and the VecEnv wrappers' base driven with a stub env."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from quadruped_gym_amd import _abi, curriculum, schedule, shaped, task_layers
from quadruped_gym_amd._handle import Handle
from quadruped_gym_amd.envs.device_wrapper import STEP_BUFFERS, DeviceVecEnvWrapper

from helpers import header_define, header_text

LAYERS = ("NORM", "ROLLOUT", "PERTURB", "CONTACT")


def test_the_four_done_pairs_are_the_one():
    header = header_text()
    assert (header_define(header, "QG_DONE_U8"), header_define(header, "QG_DONE_F32")) == (_abi.DONE_U8, _abi.DONE_F32) == (0, 1)
    for layer in LAYERS:
        for kind in ("U8", "F32"):
            assert f"#define QG_{layer}_DONE_{kind} QG_DONE_{kind}" in header                      # an alias, not a second literal
            assert header_define(header, f"QG_{layer}_DONE_{kind}") == header_define(header, f"QG_DONE_{kind}")
            assert getattr(_abi, f"{layer}_DONE_{kind}") == getattr(_abi, f"DONE_{kind}")


def test_one_prototype_table_is_exports_and_the_binding():
    assert _abi.EXPORTS == tuple(_abi.PROTOTYPES) and len(set(_abi.EXPORTS)) == len(_abi.EXPORTS) > 100
    lib = _abi.load_library()
    marked = {}
    for name, proto in _abi.PROTOTYPES.items():
        argtypes, restype = proto if isinstance(proto, tuple) else (proto, C.c_int)
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name
        assert fn.restype is restype, name
        if isinstance(proto, tuple):
            marked[name] = restype
    # the entry points whose result is not the int status, as include/quadgym.h declares them
    assert marked == {"qg_version": C.c_char_p, "qg_build_id": C.c_char_p, "qg_last_error": C.c_char_p, "qg_recommended_batch": C.c_int32,
                      "qg_time_limit_substeps": C.c_int64, "qg_walk_state_bytes": C.c_int64, "qg_po_state_bytes": C.c_int64,
                      "qg_contact_state_bytes": C.c_int64}
    header = header_text()
    for name, restype in marked.items():
        c_type = {C.c_char_p: "const char *", C.c_int32: "int32_t ", C.c_int64: "int64_t "}[restype]
        assert f"{c_type}{name}(" in header, name


def _sized_classes():
    found, todo = [], [_abi._Sized]
    while todo:
        for cls in todo.pop().__subclasses__():
            found.append(cls)
            todo.append(cls)
    return found


def test_every_struct_with_a_struct_size_is_sized():
    sized = _sized_classes()
    everywhere = {id(v): v for module in (_abi, schedule, curriculum) for v in vars(module).values()}.values()       # a class once
    with_field = [v for v in everywhere if isinstance(v, type) and issubclass(v, C.Structure) and v is not _abi._Sized
                  and "struct_size" in [f[0] for f in getattr(v, "_fields_", [])]]
    assert sorted(c.__name__ for c in with_field) == sorted(c.__name__ for c in sized) and len(sized) == 16
    assert schedule.QgSchedDesc is _abi.QgSchedDesc and curriculum.QgCmdCurDesc is _abi.QgCmdCurDesc
    for cls in sized:
        assert cls._fields_[0][0] == "struct_size"


@pytest.mark.parametrize("make", [
    lambda: _abi.QgPolicyDesc.make(33, (64, 64), 12), lambda: _abi.QgPpoParams.make(), lambda: _abi.QgPpoBatch.make(33, obs=16),
    lambda: _abi.QgAdamParams.make(), lambda: _abi.QgNormDesc.make(33, 8), lambda: _abi.QgRolloutDesc.make(8, 4, 33, 12),
    lambda: _abi.QgRolloutStorage.make(), lambda: _abi.QgRolloutStep.make(done_stride=1), lambda: _abi.QgRolloutBatch.make(),
    lambda: _abi.QgPerturbDesc.make(8, 33), lambda: _abi.QgContactDesc.make(1.5), lambda: _abi.QgGaitDesc.make(),
    lambda: _abi.QgDistillParams.make("kl", 0.25), lambda: _abi.QgDistillBatch.make(33, obs=16), lambda: _abi.QgSchedDesc.make(),
    lambda: _abi.QgCmdCurDesc.make()],
    ids=["policy_desc", "ppo_params", "ppo_batch", "adam_params", "norm_desc", "rollout_desc", "rollout_storage", "rollout_step",
         "rollout_batch", "perturb_desc", "contact_desc", "gait_desc", "distill_params", "distill_batch", "sched_desc", "cmdcur_desc"])
def test_make_fills_struct_size(make):
    d = make()
    assert isinstance(d, _abi._Sized) and d.struct_size == C.sizeof(type(d)) > 0


def test_make_keeps_each_structs_own_conversions():
    d = _abi.QgPolicyDesc.make(33, (64, 32), 12, out_tanh=True, value=False)
    assert (d.obs_dim, d.act_dim, d.n_hidden, list(d.hidden), d.out_tanh, d.has_value) == (33, 12, 2, [64, 32, 0], 1, 0)
    b = _abi.QgPpoBatch.make(35, obs=4096, returns=8192)
    assert (b.obs_stride, b.obs, b.returns, b.actions) == (35, 4096, 8192, None)
    assert _abi.QgPpoParams.make(clip_range_vf=None).clip_range_vf == 0.0 and _abi.QgAdamParams.make(max_grad_norm=None).max_grad_norm == 0.0
    p = _abi.QgPerturbDesc.make(8, 26, window=5, delays=(1, 3), max_delay=3, obs_std=[0.5], seed=-1)
    assert (p.n_envs, p.frame_dim, p.window, p.delay_lo, p.delay_hi, p.obs_std[0], p.obs_std[1], p.seed) == (8, 26, 5, 1, 3, 0.5, 0.0, 2**64 - 1)
    assert _abi.QgContactDesc.make(2).force_threshold == 2.0
    g = _abi.QgGaitDesc.make(range(1, 8), 0.25, 0.5, 20, 0.125)              # weights in GAIT_TERMS order, the four thresholds
    assert (list(g.weights), g.air_time_target, g.clearance_target, g.max_contact_force, g.min_command_speed, g.reserved) == (
        [1, 2, 3, 4, 5, 6, 7], 0.25, 0.5, 20.0, 0.125, 0) and len(g.weights) == len(_abi.GAIT_TERMS)
    s = _abi.QgSchedDesc.make((((0.0, 0.5, 0.0, 0.5), 0.5), ((0.0, 0.5, 0.75, 0.25), 0.75)), (1.0, 3.0), [1, 2, 3, 4], random_phase=True, seed=-1)
    assert (s.n_gaits, list(s.gaits[1].offset), s.gaits[1].duty, list(s.gaits[2].offset), s.freq_lo, s.freq_hi, list(s.weights)) == (
        2, [0.0, 0.5, 0.75, 0.25], 0.75, [0.0] * 4, 1.0, 3.0, [1, 2, 3, 4])
    assert (s.seed, s.random_phase, _abi.QgSchedDesc.make(random_phase=0).random_phase, s.reserved) == (2 ** 64 - 1, 1, 0, 0)
    c = _abi.QgCmdCurDesc.make((0.0, 2.0), (2, 3), [1] * 6, 8, 2, criteria=((3, 1, 0.5), (10, -1, -0.25)), fixed_heading=None)
    assert (c.n_speed, c.n_alpha, c.n_criteria, c.fixed_heading, c.heading_angle, list(c.initial_weights[:7])) == (2, 3, 2, 0, 0.0, [1] * 6 + [0])
    assert [(r.column, r.sense, r.threshold) for r in c.criteria[:3]] == [(3, 1, 0.5), (10, -1, -0.25), (0, 0, 0.0)]
    h = _abi.QgCmdCurDesc.make(fixed_heading=0.5)
    assert (h.fixed_heading, h.heading_angle) == (1, 0.5)


# -- the one strided-rows check with a stub tensor: no device ------------------------------------------------------------------------
class _StubTensor:
    def __init__(self, shape, strides, dtype="float32", cuda=True, index=0):
        import torch
        self.shape, self._strides, self.dtype, self.is_cuda = tuple(shape), tuple(strides), getattr(torch, dtype), cuda
        self.device = type("_Device", (), {"index": index})()
        self._ptr = 0

    def dim(self):
        return len(self.shape)

    def stride(self, k=None):
        return self._strides if k is None else self._strides[k]

    def data_ptr(self):
        return self._ptr

    def at(self, ptr):
        self._ptr = ptr
        return self


def _stub_handle():
    h = object.__new__(Handle)                          # no library handle: the checks read these three attributes only
    h.device, h.num_envs, h.obs_dim = 0, 3, 5
    return h


@pytest.mark.parametrize("shape, strides, want", [((3, 5), (5, 1), 5), ((3, 5), (8, 1), 8), ((1, 5), (0, 1), 5), ((3, 1), (2, 2), 2)],
                         ids=["contiguous", "column_slice", "one_row", "width_one_strided"])
def test_check_rows_accepts_strided_rows_and_returns_the_stride(shape, strides, want):
    h = _stub_handle()
    t = _StubTensor(shape, strides)
    assert h._check_rows(t, shape[1], "x", rows=shape[0]) == want
    if shape[0] == h.num_envs:
        assert h._check_rows(t, shape[1], "x") == want                     # rows defaults to num_envs
    assert h._check_rows(t, shape[1], "x", rows=Handle.ANY_ROWS) == want


@pytest.mark.parametrize("tensor, message", [
    (_StubTensor((3, 5), (5, 1), cuda=False), "x must live on cuda:0"),
    (_StubTensor((3, 5), (5, 1), index=1), "x must live on cuda:0"),
    (_StubTensor((3, 5), (5, 1), dtype="float64"), "x: expected a float32 tensor of shape (3, 5), got torch.float64 (3, 5)"),
    (_StubTensor((15,), (1,)), "x: expected a float32 tensor of shape (3, 5), got torch.float32 (15,)"),
    (_StubTensor((3, 5, 1), (5, 1, 1)), "x: expected a float32 tensor of shape (3, 5), got torch.float32 (3, 5, 1)"),
    (_StubTensor((4, 5), (5, 1)), "x: expected a float32 tensor of shape (3, 5), got torch.float32 (4, 5)"),
    (_StubTensor((3, 4), (4, 1)), "x: expected a float32 tensor of shape (3, 5), got torch.float32 (3, 4)"),
    (_StubTensor((3, 5), (4, 1)), "x: rows must be contiguous, at a row stride >= 5; got strides (4, 1)"),
    (_StubTensor((3, 5), (1, 3)), "x: rows must be contiguous, at a row stride >= 5; got strides (1, 3)"),
    (_StubTensor((3, 5), (0, 1)), "x: rows must be contiguous, at a row stride >= 5; got strides (0, 1)")],
    ids=["not_cuda", "other_device", "float64", "one_dim", "three_dim", "row_count", "width", "rows_overlap", "transposed", "expanded"])
def test_check_rows_refuses_with_the_three_message_shapes(tensor, message):
    with pytest.raises(ValueError) as err:
        _stub_handle()._check_rows(tensor, 5, "x")
    assert str(err.value) == message


def test_check_obs_is_check_rows_at_obs_dim():
    h = _stub_handle()
    assert h._check_obs(_StubTensor((3, 5), (8, 1))) == (3, 8) == h._check_obs(_StubTensor((3, 5), (8, 1)), 3)
    assert h._check_obs(_StubTensor((7, 5), (5, 1))) == (7, 5) and h._check_obs(_StubTensor((1, 5), (0, 1))) == (1, 5)     # any n >= 1
    for bad, n, message in ((_StubTensor((7, 5), (5, 1)), 3, "next_obs: expected a float32 tensor of shape (3, 5), got torch.float32 (7, 5)"),
                            (_StubTensor((0, 5), (5, 1)), None, "next_obs: expected a float32 tensor of shape (n, 5), got torch.float32 (0, 5)"),
                            (_StubTensor((3, 5), (5, 2)), None, "next_obs: rows must be contiguous, at a row stride >= 5; got strides (5, 2)")):
        with pytest.raises(ValueError) as err:
            h._check_obs(bad, n, "next_obs")
        assert str(err.value) == message
    h.obs_dim = 1                                       # the widened case: a single column has no inner stride to violate
    assert h._check_obs(_StubTensor((3, 1), (2, 2))) == (3, 2)


# -- a task layer's state size in the ABI's two forms, with a fake library ----------------------------------------------------------------
class _SizeLib:
    """`size` as qg_walk_state_bytes returns it (the result) and as qg_sched_state_bytes does (through the pointer, beside `status`)."""

    def __init__(self, size, status=0):
        self.size, self.status, self.calls = size, status, []

    def qg_walk_state_bytes(self, h):
        self.calls.append(("result", h))
        return self.size

    def qg_sched_state_bytes(self, h, out):
        self.calls.append(("pointer", h))
        out._obj.value = self.size
        return self.status


def _layer(prefix, lib):
    layer = object.__new__(task_layers._TaskLayer)
    layer._abi_prefix, layer._lib, layer._h = prefix, lib, "handle"
    return layer


def test_state_bytes_reads_the_entry_points_form_from_the_prototype_table(monkeypatch):
    forms = {name: isinstance(proto, tuple) for name, proto in _abi.PROTOTYPES.items() if name.endswith("_state_bytes")}
    assert forms == {"qg_walk_state_bytes": True, "qg_po_state_bytes": True, "qg_contact_state_bytes": True, "qg_sched_state_bytes": False,
                     "qg_cmdcur_state_bytes": False}
    assert list(_abi.PROTOTYPES["qg_sched_state_bytes"]) == [C.c_void_p, C.POINTER(C.c_int64)] == list(_abi.PROTOTYPES["qg_cmdcur_state_bytes"])
    assert "state_bytes" not in vars(schedule.GaitSchedule) and "state_bytes" not in vars(curriculum.CommandCurriculum)     # the one reader
    failed = []
    monkeypatch.setattr(task_layers, "check", lambda status, what: status and failed.append((status, what)))     # the refusals only
    for prefix, form in (("qg_walk", "result"), ("qg_sched", "pointer")):
        lib = _SizeLib(4096)
        assert _layer(prefix, lib).state_bytes() == 4096 and lib.calls == [(form, "handle")] and failed == []
    # the error path of each: a status below zero as the result; a status beside a size that was never written
    for size in (-1, -3, 0):
        _layer("qg_walk", _SizeLib(size)).state_bytes()
    assert failed == [(-1, "qg_walk_state_bytes"), (-3, "qg_walk_state_bytes"), (-1, "qg_walk_state_bytes")]
    del failed[:]
    _layer("qg_sched", _SizeLib(0, status=-1)).state_bytes()
    assert failed == [(-1, "qg_sched_state_bytes")]
    monkeypatch.undo()
    with pytest.raises(_abi.QuadGymError, match=r"qg_sched_state_bytes failed \(-1\)"):            # and through the real check
        _layer("qg_sched", _SizeLib(0, status=-1)).state_bytes()
    with pytest.raises(_abi.QuadGymError, match=r"qg_walk_state_bytes failed \(-2\)"):
        _layer("qg_walk", _SizeLib(-2)).state_bytes()


# -- the shaped-reward layers' arguments with stub tensors: no device ------------------------------------------------------------------------
def _shaped_layer(terms):
    layer = type("_Layer", (shaped.ShapedReward, Handle), {"TERMS": terms})
    h = object.__new__(layer)
    h.device, h.num_envs = 0, 3
    return h


SHAPED = [(_abi.GAIT_TERMS, 7, 25), (_abi.SCHED_TERMS, 4, 28)]


@pytest.mark.parametrize("terms, nt, limit", SHAPED, ids=["gait", "schedule"])
def test_shaped_args_returns_the_tensors_pointers_and_strides(terms, nt, limit):
    assert len(terms) == nt and _abi.MONITOR_MAX_TERMS - nt == limit
    h, c0 = _shaped_layer(terms), 11
    done = _StubTensor((3,), (35,), dtype="uint8").at(0x100)
    reward, out = _StubTensor((3,), (35,)).at(0x200), _StubTensor((3,), (2,)).at(0x300)
    wide = _StubTensor((3, c0 + nt), (40, 1)).at(0x1000)
    base, command = _StubTensor((3, c0), (16, 1)).at(0x4000), _StubTensor((3, 2), (260, 1)).at(0x5000)
    seen = []
    done3, rows11, comps, rew = h._shaped_args(done, reward, out, wide, base, command, lambda: seen.append("also"))
    assert done3 == (0x100, _abi.DONE_U8, 35) and comps is wide and rew is out and seen == ["also"]
    assert rows11 == (0x200, 35, 0x300, 2, 0x1000, 40, 0x4000, 16, c0, 0x5000, 260)
    # base as components[:, :C0] in place: the same rows at the same stride, at the limit of the width too
    for width in (c0, limit):
        wide = _StubTensor((3, width + nt), (64, 1)).at(0x1000)
        _, rows11, _, _ = h._shaped_args(None, None, out, wide, _StubTensor((3, width), (64, 1)).at(0x1000), None)
        assert rows11 == (None, 1, 0x300, 2, 0x1000, 64, 0x1000, 64, width, None, 2)
    # no base: the layer's own columns alone
    assert h._shaped_args(None, None, out, _StubTensor((3, nt), (nt, 1)).at(0x1000), None, None)[1][4:9] == (0x1000, nt, None, 0, 0)


@pytest.mark.parametrize("terms, nt, limit", SHAPED, ids=["gait", "schedule"])
def test_shaped_args_refuses_before_it_allocates(terms, nt, limit):
    h, c0 = _shaped_layer(terms), 11
    out = _StubTensor((3,), (1,)).at(0x300)
    wide = lambda ptr=0x1000, stride=40: _StubTensor((3, c0 + nt), (stride, 1)).at(ptr)
    overlap = "base_components and components overlap: allowed only where base_components is components[:, :C0]"
    too_wide = f"base_components: expected [N, C0] with C0 <= {limit}, got (3, {limit + 1})"
    for kw, message in (
            # the base behind the front of the same buffer (columns 4 .. 4 + C0 of the wide rows) ...
            (dict(components=wide(), base_components=_StubTensor((3, c0), (40, 1)).at(0x1000 + 16)), overlap),
            # ... the same columns at another stride, and rows that merely end inside the wide buffer
            (dict(components=wide(), base_components=_StubTensor((3, c0), (c0, 1)).at(0x1000)), overlap),
            (dict(components=wide(), base_components=_StubTensor((3, c0), (c0, 1)).at(0x1000 - 4 * (2 * c0 + 1))), overlap),
            (dict(base_components=_StubTensor((3, limit + 1), (limit + 1, 1))), too_wide),
            (dict(components=wide(), base_components=_StubTensor((3, c0), (c0, 1), cuda=False)), "base_components must live on cuda:0"),
            (dict(components=_StubTensor((3, nt), (nt, 1), cuda=False)), "components must live on cuda:0"),
            (dict(reward=_StubTensor((3,), (1,), cuda=False)), "reward must live on cuda:0"),
            (dict(command=_StubTensor((3, 2), (2, 1), cuda=False)), "command must live on cuda:0"),
            (dict(done=_StubTensor((3,), (1,), dtype="uint8", cuda=False)), "done must live on cuda:0")):
        with pytest.raises(ValueError) as err:                          # (nothing is allocated: an allocation would need a device)
            h._shaped_args(**dict(dict(done=None, reward=None, reward_out=out, components=None, base_components=None, command=None), **kw))
        assert str(err.value) == message, kw
    # disjoint rows pass: the base ends where the wide rows begin
    ok = _StubTensor((3, c0), (c0, 1)).at(0x1000 - 4 * 3 * c0)
    assert h._shaped_args(None, None, out, wide(), ok, None)[1][6:9] == (0x1000 - 4 * 3 * c0, c0, c0)
    with pytest.raises(ValueError, match="unknown reward terms \\['nope'\\]: one of " + terms[0]):
        shaped.term_weights({"nope": 1.0}, terms)
    assert shaped.term_weights({terms[-1]: 2}, terms) == [0.0] * (nt - 1) + [2.0]


# -- the layers' C code -------------------------------------------------------------------------------------------------------------------
def test_layer_helpers_exist_once():
    """The f64 moments (Chan's merge, the shifted-sums finish), the finite test of a double and the lifetime of a host staging buffer
    are text of qg_moments_dev.h and qg_host.h, not a copy per layer: each fragment occurs there only, among the .hip / .h / .inc files
    of csrc/.  A copy that has to stay for its listing's sake (tools/asm_diff.py) would be named here with its reason: there is none."""
    csrc = os.path.join(_abi.package_dir(), "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".inc"))}

    def files(pattern):
        return [f for f, t in text.items() if re.search(pattern, t)]

    # Chan's merge and the finish of the shifted sums
    assert files(re.escape("d * d * na * f")) == ["qg_moments_dev.h"] == files(re.escape("s2 - s1 * s1 / cnt"))
    assert files(re.escape('#include "qg_moments_dev.h"')) == ["qg_monitor.hip", "qg_norm.hip"]
    # the exponent test of a double
    assert files(re.escape("0x7ff) != 0x7ff")) == ["qg_host.h"]
    # host staging buffers are QgHostBuf's: no translation unit allocates or frees one by hand (qg_resident_free( is a function's name)
    for pattern in (r"new \(std::nothrow\) [^;(]*\[", r"delete\s*\[\]", r"(?<![A-Za-z0-9_])malloc\(", r"(?<![A-Za-z0-9_])free\("):
        assert [f for f in files(pattern) if f.endswith(".hip")] == [], pattern
    assert files(r"new \(std::nothrow\) [^;(]*\[") == ["qg_host.h"] == files(r"delete\s*\[\]")
    # one alignment test
    assert files(r"rollout_aligned|qga_aligned16|\(uintptr_t\)feet & 15") == []


def test_shaped_tail_exists_once():
    """The tail of a shaped-reward launch (weigh the terms, zero a finished env, ascending sum, one component per lane, base columns
    copied, reward added with a finished env passing through), the host's checks of its arguments and the Python plumbing in front of
    them are text of csrc/qg_shaped_dev.h and shaped.py that the gait reward and the gait schedule use, not a copy per layer.  What
    stays a copy for its listing's sake (tools/asm_diff.py) is named at the end with its reason."""
    csrc = os.path.join(_abi.package_dir(), "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".inc"))}
    header, users = ["qg_shaped_dev.h"], ["qg_gait.hip", "qg_sched.hip"]

    def files(needle):
        return [f for f, t in text.items() if needle in t]

    for needle in ("mine = lane == k ? comp[k] : mine",                 # one component per lane
                   "r = finished ? r0 : ADD(r0, shaped)",              # the finished env's reward passes through
                   "finished ? 0.f : MUL(",                            # ... and its components are zeros
                   "base_components and components overlap", "base_terms %d without base_components", "reward without reward_out",
                   "components_stride %d must be >= base_terms", "weights[%d] is not finite", "fmaxf(fabsf(", "struct KShapedIO"):
        assert files(needle) == header, needle
    assert files("finished ? r0 :") == header and files("check_weights(const float") == header
    assert files('#include "qg_shaped_dev.h"') == users == files("KShapedIO io;")
    for macro in ("QG_SHAPED_WEIGH(", "QG_SHAPED_STORE("):              # each kernel expands each macro exactly once
        assert {f: t.count(macro) for f, t in text.items() if macro in t} == {"qg_gait.hip": 1, "qg_sched.hip": 1, "qg_shaped_dev.h": 1}, macro
    assert text["qg_gait.hip"].count("__fmul_rn, __fadd_rn") == 1 and text["qg_sched.hip"].count("QGS_MUL, QGS_ADD") == 1      # own spelling
    assert files("qg_shaped_io(") == users + header and all(text[f].count("qg_shaped_io(") == 1 for f in users + header)
    # the Python side: the package's .py files
    package = {}
    for top, _, names in os.walk(_abi.package_dir()):
        package.update({os.path.relpath(os.path.join(top, f), _abi.package_dir()): open(os.path.join(top, f)).read()
                        for f in names if f.endswith(".py")})
    for needle in ("unknown reward terms", "PO_COMMAND = 23", "allowed only where base_components is components[:, :C0]",
                   "only the partially observable env's observation holds the command", "def _span("):
        assert [f for f, t in package.items() if needle in t] == ["shaped.py"], needle
    assert [f for f, t in package.items() if "struct_size = C.sizeof(cls)" in t] == ["_abi.py"]
    # left unshared: the ascending sum over the foot lanes 3, 6, 9, 12.  One expression per summed value, or one loop per value, in
    # place of the kernels' one loop over the feet with every value inside, changes the register assignment of all four reward
    # kernels (docs/EXPERIMENTS.md, "The shaped-reward tail"), so each kernel keeps its loop.
    assert files("for (int src = 6; src <= 12; src += 3)") == users


# -- the wrappers' base with a stub env: no library call -------------------------------------------------------------------------------
class _StubEnv:
    packed_step = False
    num_envs = 3
    obs_dim = 5

    def __init__(self):
        self.calls = []

    def snapshot(self):
        return {"sim": "state"}

    def restore(self, snap):
        self.calls.append(("restore", snap))

    def close(self):
        self.calls.append("close")

    def step_async(self, actions):
        self.calls.append(("step_async", actions))


class _StubLayer:
    def __init__(self, calls):
        self.calls = calls

    def close(self):
        self.calls.append("layer close")


class _Wrapper(DeviceVecEnvWrapper):
    _snapshot_key = "layer"
    state = 7

    def _layer_state(self):
        return self.state

    def _load_layer_state(self, state):
        self.state = state

    def step_wait(self):
        return "waited"


def test_wrapper_passes_through_and_does_not_recurse_before_venv_is_set():
    env = _StubEnv()
    w = _Wrapper(env, _StubLayer(env.calls))
    assert w.venv is env and w.num_envs == 3 and w.obs_dim == 5 and w._packed is False
    with pytest.raises(AttributeError):
        w.no_such_attribute
    bare = object.__new__(_Wrapper)                     # what copy / pickle do: no __init__ has run
    with pytest.raises(AttributeError):
        bare.venv
    with pytest.raises(AttributeError):
        bare.num_envs
    assert w.step("a") == "waited" and env.calls == [("step_async", "a")]


def test_step_buffers_binds_positional_and_keyword_buffers_alike():
    assert STEP_BUFFERS == ("obs", "reward", "done", "components", "terminal_obs")
    o, r, d, c, t = (object() for _ in range(5))
    want = {"obs": o, "reward": r, "done": d, "components": c, "terminal_obs": t}
    bind = DeviceVecEnvWrapper._step_buffers
    assert bind((o, r, d, c, t), {}) == want
    assert bind((), dict(want, stream="s")) == want
    assert bind((o, r), {"done": d, "terminal_obs": t, "stream": None}) == {"obs": o, "reward": r, "done": d, "terminal_obs": t}
    assert bind((o, r, d), {}).get("terminal_obs") is None


def test_finished_with_terminal_skips_infos_without_one():
    term = np.ones(5, np.float32)
    done = np.array([1, 0, 1, 1, 1, 0], np.uint8)
    infos = [{"terminal_observation": term}, {"terminal_observation": term}, {}, None, {"terminal_observation": None, "x": 1},
             {"terminal_observation": term}]
    assert DeviceVecEnvWrapper._finished_with_terminal(done, infos) == [(0, infos[0])]
    done[5] = 1
    picked = DeviceVecEnvWrapper._finished_with_terminal(done.astype(bool), infos)
    assert [i for i, _ in picked] == [0, 5] and all(type(i) is int for i, _ in picked) and picked[1][1] is infos[5]
    assert DeviceVecEnvWrapper._finished_with_terminal(np.zeros(6, bool), infos) == []


def test_snapshot_restore_close_go_through_the_two_hooks():
    env = _StubEnv()
    w = _Wrapper(env, _StubLayer(env.calls))
    snap = w.snapshot()
    assert snap == {"env": {"sim": "state"}, "layer": 7}
    w.state = 8
    w.restore(snap)
    assert w.state == 7 and env.calls == [("restore", {"sim": "state"})]
    w.close()
    assert env.calls[1:] == ["layer close", "close"]                    # the layer first, then the env it reads
