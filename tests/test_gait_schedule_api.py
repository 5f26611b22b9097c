"""The gait schedule without a GPU: its entry points exist in the library, the header and the binding; the descriptor's ctypes mirror
has the C layout; the term and column names are the header's QG_SCHED_*; bad descriptors and NULL handles are refused with QG_ERR_ARG
before any device call; bad Python arguments raise ValueError before the library is reached; and the wrapper refuses, at construction
and before any handle is created, the stacks that cannot work -- naming the order that does."""
import ctypes as C
import math
import os
import shutil
import subprocess
from types import SimpleNamespace

import pytest

from quadruped_gym_amd import _abi, schedule
from quadruped_gym_amd.envs.device_wrapper import DeviceVecEnvWrapper
from quadruped_gym_amd.normalize import DeviceVecNormalize
from quadruped_gym_amd.perturb import DevicePerturbedVecEnv
from quadruped_gym_amd.privileged import DevicePrivilegedVecEnv
from quadruped_gym_amd.schedule import GAITS, DeviceGaitScheduleVecEnv, GaitSchedule, QgSchedDesc, gait_table, term_weights

import gait_schedule_reference as R
from helpers import header_define

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QG_ERR_ARG = -1
NEW = ("qg_sched_create", "qg_sched_destroy", "qg_sched_set_weights", "qg_sched_advance_device", "qg_sched_begin_device", "qg_sched_get_gaits",
       "qg_sched_state_bytes", "qg_sched_get_state", "qg_sched_set_state")
N = 8


def _header():
    return open(os.path.join(ROOT, "include", "quadgym.h")).read()


def test_symbols_are_exported_declared_and_bound():
    lib, header = _abi.load_library(), _header()
    for name in NEW:
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"int {name}(" in header
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    for word in ("typedef struct qg_sched_desc", "THE SENSOR'S TIMERS AND ARMED FLAGS ARE NEITHER READ NOR WRITTEN", "0x5147534348454431",
                 "qg_resident_stop first", "Destroy the qg_sched before its qg_contact", "freq_hi * dt32 > 0.5"):
        assert word in header, word
    for method in ("step", "begin", "gaits", "set_weights", "state", "load_state", "close"):
        assert callable(getattr(GaitSchedule, method))
    for method in ("step_tensor", "step_wait", "reset", "snapshot", "restore", "close"):
        assert callable(getattr(DeviceGaitScheduleVecEnv, method))
    csrc = os.path.join(ROOT, "quadruped-gym_amd", "csrc")
    assert "qg_sched" in open(os.path.join(csrc, "Makefile")).read().split("TUS =")[-1].split("OBJS")[0]
    text = open(os.path.join(csrc, "qg_sched.hip")).read()
    # the sensor's device code and the perturbation layer's hash are shared, not copied; no profiling-build names
    assert '#include "qg_contact_dev.h"' in text and '#include "qg_key_dev.h"' in text and "0xBF58476D1CE4E5B9" not in text
    assert '#include "qg_key_dev.h"' in open(os.path.join(csrc, "qg_perturb.hip")).read()
    assert "phase_clock" not in text.lower() and "phase clock" not in text.lower()


def test_names_are_the_headers():
    header = _header()
    assert GaitSchedule.TERMS == _abi.SCHED_TERMS == R.TERMS and len(R.TERMS) == header_define(header, "QG_SCHED_NTERMS") == 4
    for name in R.TERMS:
        assert R.TERMS[header_define(header, "QG_SCHED_" + name.upper())] == name
    assert _abi.SCHED_MAX_BASE_TERMS == header_define(header, "QG_MONITOR_MAX_TERMS") - 4 == 28
    assert _abi.SCHED_DIM == header_define(header, "QG_SCHED_DIM") == 10 == sum(w for _, _, w in _abi.SCHED_COLUMNS)
    assert [first for _, first, _ in _abi.SCHED_COLUMNS] == [header_define(header, "QG_SCHED_" + k) for k in ("SIN", "COS", "FREQ", "DUTY")]
    assert _abi.SCHED_MAX_GAITS == header_define(header, "QG_SCHED_MAX_GAITS") == 8
    assert schedule.DONE_ROWS == {"reset": header_define(header, "QG_PERTURB_DONE_ROW_RESET"),
                                  "terminal": header_define(header, "QG_PERTURB_DONE_ROW_TERMINAL")}


def _good():
    return QgSchedDesc.make(R.TABLE, R.FREQ, [1, -1, 1, -1], True, 1, seed=5, env_index_base=3, **R.LIMITS)


def _create(desc, contact=None):
    lib = _abi.load_library()
    h = C.c_void_p()
    rc = lib.qg_sched_create(contact, C.byref(desc) if desc is not None else None, C.byref(h))
    assert not h.value
    return rc, lib.qg_last_error().decode()


def test_mirror_has_the_c_layout(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler to build the sizeof probe with")
    fields = [f for f, _ in QgSchedDesc._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "quadgym.h"\nint main(void) {\n    printf("%zu", sizeof(qg_sched_desc));\n'
                   + "".join(f'    printf(" %zu", offsetof(qg_sched_desc, {f}));\n' for f in fields)
                   + '    printf(" %zu %zu", sizeof(qg_sched_gait), offsetof(qg_sched_gait, duty));\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(s) for s in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(QgSchedDesc)] + [getattr(QgSchedDesc, f).offset for f in fields] + [C.sizeof(schedule.QgSchedGait), 16]
    d = _good()
    assert got[0] == 240 == d.struct_size and d.reserved == 0 and d.n_gaits == 5 and d.random_phase == 1 and d.done_row == 1
    assert list(d.weights) == [1, -1, 1, -1] and (d.seed, d.env_index_base) == (5, 3)
    assert list(d.gaits[4].offset) == [0.0, 0.5, 0.75, 0.25] and d.gaits[4].duty == 0.75 and d.gaits[5].duty == 0.0
    assert (d.freq_lo, d.freq_hi, d.kappa) == (1.0, 3.0, 1.0 / 256)
    assert QgSchedDesc.make(seed=-1).seed == 2 ** 64 - 1


def test_bad_descriptors_are_refused_before_any_device_call():
    lib = _abi.load_library()
    assert lib.qg_sched_create(None, C.byref(_good()), None) == QG_ERR_ARG
    assert _create(None)[0] == QG_ERR_ARG
    put = lambda field, value: (lambda d: setattr(d, field, value))
    bad = {"struct_size": lambda d: setattr(d, "struct_size", d.struct_size + 8), "reserved": put("reserved", 1),
           "n_gaits 0": put("n_gaits", 0), "n_gaits 9": put("n_gaits", 9), "random_phase": put("random_phase", 2),
           "done_row": put("done_row", 2), "frequencies 0": put("freq_lo", 0.0), "frequencies -": put("freq_lo", -1.0),
           "frequencies order": put("freq_hi", 0.5), "frequencies nan": put("freq_hi", math.nan), "frequencies inf": put("freq_hi", math.inf),
           "kappa -": put("kappa", -1e-3), "kappa wide": put("kappa", 1.0 / 64), "kappa nan": put("kappa", math.nan),
           "sigma_force 0": put("sigma_force", 0.0), "sigma_force nan": put("sigma_force", math.nan),
           "sigma_velocity -": put("sigma_velocity", -1.0), "sigma_velocity inf": put("sigma_velocity", math.inf),
           "swing_height_target": put("swing_height_target", math.nan), "min_command_speed -": put("min_command_speed", -0.1),
           "min_command_speed nan": put("min_command_speed", math.nan)}
    for k in (0, 3):
        bad["weights[%d] nan" % k] = lambda d, k=k: d.weights.__setitem__(k, math.nan)
    for g in (0, 4):
        bad["gaits[%d].offset[3] 1" % g] = lambda d, g=g: d.gaits[g].offset.__setitem__(3, 1.0)
        bad["gaits[%d].offset[0] -" % g] = lambda d, g=g: d.gaits[g].offset.__setitem__(0, -0.25)
        bad["gaits[%d].duty low" % g] = lambda d, g=g: setattr(d.gaits[g], "duty", 1.0 / 128)
        bad["gaits[%d].duty high" % g] = lambda d, g=g: setattr(d.gaits[g], "duty", 0.99)
        bad["gaits[%d].duty nan" % g] = lambda d, g=g: setattr(d.gaits[g], "duty", math.nan)
    for word, spoil in bad.items():
        d = _good()
        spoil(d)
        rc, msg = _create(d)
        assert rc == QG_ERR_ARG and word.split()[0] in msg, (word, rc, msg)
    unused = _good()                                          # rows past n_gaits are not looked at
    unused.gaits[6].duty = math.nan
    for d in (_good(), unused):                               # a good one gets as far as the sensor it is bound to
        rc, msg = _create(d)
        assert rc == QG_ERR_ARG and "null contact sensor" in msg


def test_null_handles_are_refused():
    lib = _abi.load_library()
    buf = (C.c_float * 64)()
    n64 = C.c_int64()
    assert lib.qg_sched_destroy(None) == 0                    # as every destroy of the library
    assert lib.qg_sched_set_weights(None, buf) == QG_ERR_ARG
    assert lib.qg_sched_advance_device(None, None, 0, 1, None, 1, buf, 1, buf, 4, None, 0, 0, None, 2, None, 0, 0, None, 0, None, 0, None, 0,
                                    None) == QG_ERR_ARG
    assert b"null handle" in lib.qg_last_error()
    assert lib.qg_sched_begin_device(None, None, None, 0, 0, None) == QG_ERR_ARG
    assert lib.qg_sched_get_gaits(None, buf, buf, buf) == QG_ERR_ARG
    assert lib.qg_sched_state_bytes(None, C.byref(n64)) == QG_ERR_ARG and lib.qg_sched_get_state(None, buf) == QG_ERR_ARG
    assert lib.qg_sched_set_state(None, buf) == QG_ERR_ARG


class _Sensor:
    """What GaitSchedule reads of a ContactSensor before it reaches the library."""
    device, num_envs, _h = 0, N, None


def _unbound(n=N, done_row="reset"):
    """A GaitSchedule that has no handle: every check of step() that precedes the library can be reached without a GPU."""
    g = object.__new__(GaitSchedule)
    g.device, g.num_envs, g._h, g._lib, g.done_row = 0, n, None, None, done_row
    return g


def test_python_refuses_bad_arguments_before_the_library():
    import torch
    assert term_weights(None) == [0.0] * 4 and term_weights({"contact_match": 2})[3] == 2.0
    assert gait_table("trot") == [GAITS["trot"]] and gait_table(["walk", ((0, 0.25, 0.5, 0.75), 0.6)])[1][1] == float(C.c_float(0.6).value)
    bad = [dict(weights={"swing_hight": 1.0}), dict(weights={"swing_force": math.nan}), dict(gaits=("gallop",)), dict(gaits=()),
           dict(gaits=("trot",) * 9), dict(gaits=[((0, 0, 0), 0.5)]), dict(gaits=[((0, 0, 0, 1.0), 0.5)]), dict(gaits=[((0, 0, 0, 0), 0.995)]),
           dict(freq=(0.0, 1.0)), dict(freq=(2.0, 1.0)), dict(freq=(1.0, math.inf)), dict(done_row="both"), dict(kappa=-0.001),
           dict(kappa=0.01), dict(sigma_force=0.0), dict(sigma_velocity=math.nan), dict(swing_height_target=math.inf),
           dict(min_command_speed=-1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            GaitSchedule(_Sensor(), **kw)
    with pytest.raises(ValueError, match="closed"):           # good arguments get as far as the sensor's handle
        GaitSchedule(_Sensor())
    g = _unbound()
    z = lambda *shape, **kw: torch.zeros(shape, **kw)
    for kw in (dict(reward=z(N)), dict(out=z(N, 10)), dict(obs=z(N, 33), out=z(N, 43)), dict(components=z(N, 4)), dict(command=z(N, 2)),
               dict(done=z(N, dtype=torch.uint8)), dict(terminal_obs=z(N, 33)), dict(base_components=z(N, 29))):
        with pytest.raises(ValueError):                       # CPU tensors, a base too wide, terminal_obs without terminal_out
            g.step(**kw)
    with pytest.raises(ValueError, match="done_row='reset'"):
        _unbound(done_row="terminal").step(terminal_out=z(N, 10))
    for kw in (dict(mask=z(N, dtype=torch.uint8)), dict(rows=z(N, 9)), dict(rows=z(N, 43), obs_dim=40)):
        with pytest.raises(ValueError):
            g.begin(**kw)


# ---- the wrapper's construction refusals, with stub envs ---------------------------------------------------------------------------------
class _Reached(Exception):
    """A wrapper's constructor got as far as creating its layer's handle."""


class _Env:
    """What the wrappers read of a batched env before they create a handle."""

    num_envs, device, frame_skip = N, 0, 4

    def __init__(self, obs_dim=33, packed_step=False, **extra):
        self.obs_dim, self.packed_step = obs_dim, packed_step
        self.model = SimpleNamespace(opt=SimpleNamespace(timestep=0.002))
        self._sim = SimpleNamespace(env_index_base=0, task=SimpleNamespace(default_ctrl=[0.0] * 12))
        self.reward_keys = ["alive_bonus"]
        self.handles = []
        self.__dict__.update(extra)

    def contact_sensor(self, force_threshold=0.0):
        self.handles.append("contact")
        return SimpleNamespace(device=0, num_envs=N, _h=None)

    def privileged_state(self, force_threshold=0.0):
        self.handles.append("privileged")
        return SimpleNamespace(device=0, num_envs=N, _h=None)


def _wrapped(cls, venv, **attrs):
    """`cls` around `venv` without its handle: what a wrapper outside it reads of it."""
    w = object.__new__(cls)
    DeviceVecEnvWrapper.__init__(w, venv, None)
    w.__dict__.update(attrs)
    return w


@pytest.fixture
def recorders(monkeypatch):
    def reached(*args, **kwargs):
        raise _Reached
    monkeypatch.setattr(schedule, "GaitSchedule", reached)
    from quadruped_gym_amd import perturb
    monkeypatch.setattr(perturb, "Perturbation", reached)


def test_wrapper_refuses_the_stacks_that_cannot_work(recorders):
    walking, po, plain = (lambda: _Env(33)), (lambda: _Env(52, FRAME=26, obs_window=2)), (lambda: _Env(33, packed_step=True))
    env = plain()
    with pytest.raises(ValueError, match=r"GaitSchedule\(env.contact_sensor\(threshold\)\).step"):
        DeviceGaitScheduleVecEnv(env)
    assert env.handles == []                                  # refused before any handle
    env = walking()
    with pytest.raises(ValueError, match=r"DevicePrivilegedVecEnv\(DeviceGaitScheduleVecEnv\(env\)\)"):
        DeviceGaitScheduleVecEnv(_wrapped(DevicePrivilegedVecEnv, env))
    with pytest.raises(ValueError, match=r"DevicePrivilegedVecEnv\(DeviceGaitScheduleVecEnv\(env\)\)"):      # ... anywhere inside it
        DeviceGaitScheduleVecEnv(_wrapped(DeviceVecNormalize, _wrapped(DevicePrivilegedVecEnv, env), normalizer=SimpleNamespace(norm_obs=False)))
    with pytest.raises(ValueError, match="only the partially observable env"):
        DeviceGaitScheduleVecEnv(env, gate_on_command=True)
    env = po()
    with pytest.raises(ValueError, match=r"DeviceVecNormalize\(DeviceGaitScheduleVecEnv\(env, gate_on_command=True\)\)"):
        DeviceGaitScheduleVecEnv(_wrapped(DeviceVecNormalize, env, normalizer=SimpleNamespace(norm_obs=True)), gate_on_command=True)
    assert env.handles == []
    # the perturbation layer around the schedule: refused by that wrapper, before its handle
    inner = _wrapped(DeviceGaitScheduleVecEnv, walking(), obs_dim=43)
    with pytest.raises(ValueError, match=r"DeviceGaitScheduleVecEnv\(DevicePerturbedVecEnv\(env\)\)"):
        DevicePerturbedVecEnv(inner)
    # the orders that work get as far as the handle
    for venv, kw in ((walking(), {}), (po(), dict(gate_on_command=True)),
                     (_wrapped(DeviceVecNormalize, po(), normalizer=SimpleNamespace(norm_obs=False)), dict(gate_on_command=True)),
                     (_wrapped(DevicePerturbedVecEnv, walking()), {})):
        with pytest.raises(_Reached):
            DeviceGaitScheduleVecEnv(venv, **kw)
    with pytest.raises(_Reached):                             # the perturbation layer inside the schedule
        DevicePerturbedVecEnv(walking())


def test_wrapper_is_ten_columns_wider():
    env = _Env(52, FRAME=26, obs_window=2)
    w = _wrapped(DeviceGaitScheduleVecEnv, env, gate_on_command=True)
    assert w.reward_keys == ["alive_bonus"] + list(R.TERMS) and w._snapshot_key == "gait_schedule"

    class _T:                                                 # what _command slices
        def __getitem__(self, key):
            return key
    assert w._command(_T()) == (slice(None), slice(26 + 23, 26 + 25))
    w.gate_on_command = False
    assert w._command(_T()) is None
