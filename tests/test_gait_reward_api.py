"""The gait reward without a GPU: its four entry points exist in the library, the header and the binding; the descriptor's ctypes mirror
has the C layout; the term names are the header's QG_GAIT_*; bad descriptors, NULL handles and bad launch arguments are refused before
any device call; bad Python arguments raise ValueError before the library is reached."""
import ctypes as C
import math
import os
import shutil
import subprocess

import pytest

from quadruped_gym_amd import _abi
from quadruped_gym_amd.gait import DeviceGaitRewardVecEnv, GaitReward, QgGaitDesc, term_weights

import gait_reward_reference as G
from helpers import header_define

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QG_ERR_ARG = -1
NEW = ("qg_gait_create", "qg_gait_destroy", "qg_gait_set_weights", "qg_gait_reward_device")


def _header():
    return open(os.path.join(ROOT, "include", "quadgym.h")).read()


def test_symbols_are_exported_declared_and_bound():
    lib, header = _abi.load_library(), _header()
    for name in NEW:
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"int {name}(" in header
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    for word in ("typedef struct qg_gait_desc", "ADVANCING READ", "does not also call qg_contact_read_device(advance = 1)",
                 "qg_resident_stop first", "destroy the qg_gait before its qg_contact"):
        assert word in header, word
    for method in ("step", "set_weights", "close"):
        assert callable(getattr(GaitReward, method))
    for method in ("step_tensor", "step_wait", "snapshot", "restore", "close"):
        assert callable(getattr(DeviceGaitRewardVecEnv, method))
    csrc = os.path.join(ROOT, "quadruped-gym_amd", "csrc")
    assert "qg_gait" in open(os.path.join(csrc, "Makefile")).read().split("TUS =")[-1].split("OBJS")[0]
    # the sensor's device code is shared, not copied
    assert '#include "qg_contact_dev.h"' in open(os.path.join(csrc, "qg_gait.hip")).read()
    assert '#include "qg_contact_dev.h"' in open(os.path.join(csrc, "qg_contact.hip")).read()


def test_term_names_are_the_headers():
    header = _header()
    assert GaitReward.TERMS == _abi.GAIT_TERMS == G.TERMS and len(G.TERMS) == header_define(header, "QG_GAIT_NTERMS") == 7
    for name in G.TERMS:
        assert G.TERMS[header_define(header, "QG_GAIT_" + name.upper())] == name
    assert _abi.GAIT_MAX_BASE_TERMS == header_define(header, "QG_MONITOR_MAX_TERMS") - 7 == 25


def _create(desc, contact=None):
    lib = _abi.load_library()
    h = C.c_void_p()
    rc = lib.qg_gait_create(contact, C.byref(desc) if desc is not None else None, C.byref(h))
    assert not h.value
    return rc, lib.qg_last_error().decode()


def _good():
    return QgGaitDesc.make([1, -1, 1, -1, 1, -1, 1], 0.02, 0.05, 20.0, 0.1)


def test_bad_descriptors_are_refused_before_any_device_call():
    lib = _abi.load_library()
    assert lib.qg_gait_create(None, C.byref(_good()), None) == QG_ERR_ARG
    assert _create(None)[0] == QG_ERR_ARG
    bad = {"struct_size": lambda d: setattr(d, "struct_size", d.struct_size + 4), "reserved": lambda d: setattr(d, "reserved", 1)}
    for k in (0, 6):
        bad["weights[%d] nan" % k] = lambda d, k=k: d.weights.__setitem__(k, math.nan)
        bad["weights[%d] inf" % k] = lambda d, k=k: d.weights.__setitem__(k, -math.inf)
    for field in ("air_time_target", "clearance_target", "max_contact_force", "min_command_speed"):
        bad[field + " -"] = lambda d, f=field: setattr(d, f, -0.5)
        bad[field + " nan"] = lambda d, f=field: setattr(d, f, math.nan)
        bad[field + " inf"] = lambda d, f=field: setattr(d, f, math.inf)
    for word, spoil in bad.items():
        d = _good()
        spoil(d)
        rc, msg = _create(d)
        assert rc == QG_ERR_ARG and word.split()[0] in msg, (word, rc, msg)
    rc, msg = _create(_good())                                # a good one gets as far as the sensor it is bound to
    assert rc == QG_ERR_ARG and "null contact sensor" in msg


def test_null_handles_are_refused():
    lib = _abi.load_library()
    buf = (C.c_float * 64)()
    assert lib.qg_gait_destroy(None) == 0                     # as every destroy of the library
    assert lib.qg_gait_set_weights(None, buf) == QG_ERR_ARG
    assert lib.qg_gait_reward_device(None, None, 0, 1, 1, None, 1, buf, 1, buf, 7, None, 0, 0, None, 2, None, None, None) == QG_ERR_ARG
    assert b"null handle" in lib.qg_last_error()


def test_mirror_has_the_c_layout(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler to build the sizeof probe with")
    fields = [f for f, _ in QgGaitDesc._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "quadgym.h"\nint main(void) {\n    printf("%zu", sizeof(qg_gait_desc));\n'
                   + "".join(f'    printf(" %zu", offsetof(qg_gait_desc, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(s) for s in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(QgGaitDesc)] + [getattr(QgGaitDesc, f).offset for f in fields]
    d = _good()
    assert got[0] == 52 == d.struct_size and d.reserved == 0 and list(d.weights) == [1, -1, 1, -1, 1, -1, 1]
    assert (d.air_time_target, d.clearance_target, d.max_contact_force, d.min_command_speed) == tuple(
        C.c_float(v).value for v in (0.02, 0.05, 20.0, 0.1))


class _Sensor:
    """What GaitReward reads of a ContactSensor before it reaches the library."""
    device, num_envs, _h = 0, 8, None


def _unbound(n=8):
    """A GaitReward that has no handle: every check of step() that precedes the library can be reached without a GPU."""
    g = object.__new__(GaitReward)
    g.device, g.num_envs, g._h, g._lib = 0, n, None, None
    return g


def test_python_refuses_bad_arguments_before_the_library():
    import torch
    assert term_weights(None) == [0.0] * 7 and term_weights({"flight": 2})[6] == 2.0
    with pytest.raises(ValueError, match="unknown reward terms"):
        GaitReward(_Sensor(), weights={"feet_airtime": 1.0})
    with pytest.raises(ValueError, match="feet_slip"):
        GaitReward(_Sensor(), weights={"feet_slip": math.nan})
    for name in ("air_time_target", "clearance_target", "max_contact_force", "min_command_speed"):
        for bad in (-1.0, math.nan, math.inf):
            with pytest.raises(ValueError, match=name):
                GaitReward(_Sensor(), weights=G.WEIGHTS, **{name: bad})
    g = _unbound()
    # tensors that do not live on the layer's device (here: the host) never reach the library (g._lib is None)
    with pytest.raises(ValueError, match="done must live on cuda:0"):
        g.step(done=torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="reward must live on cuda:0"):
        g.step(reward=torch.zeros(8))
    with pytest.raises(ValueError, match="C0 <= 25"):
        g.step(base_components=torch.zeros((8, 26)))
    with pytest.raises(ValueError, match="gate_on_command"):
        DeviceGaitRewardVecEnv(_Sensor(), gate_on_command=True)
