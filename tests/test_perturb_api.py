"""The perturbation layer without a GPU: its eight entry points exist in the library, the header and the binding; NULL handles and bad
descriptors are refused before any device call; the ctypes mirror of qg_perturb_desc has the C layout; no name reads as an env step."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import pytest

from quadruped_gym_amd import _abi
from quadruped_gym_amd import perturb as P

from helpers import header_define

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QG_ERR_ARG = -1
NEW = ("qg_perturb_create", "qg_perturb_destroy", "qg_perturb_actions_device", "qg_perturb_observe_device", "qg_perturb_begin_device",
       "qg_perturb_get_delays", "qg_perturb_get_state", "qg_perturb_set_state")


def test_symbols_are_exported_declared_and_bound():
    lib = _abi.load_library()
    header = open(os.path.join(ROOT, "include", "quadgym.h")).read()
    for name in NEW:
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"int {name}(" in header
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
        assert "step" not in name and re.fullmatch(r"qg_[a-z_]+", name)
    for word in ("typedef struct qg_perturb_desc", "0x51474E4F49534531", "QG_PERTURB_DONE_ROW_RESET", "QG_PERTURB_DONE_ROW_TERMINAL",
                 "S(f, q) = 4096 + 2 * (128 * f + q)"):
        assert word in header
    for method in ("perturb_actions", "observe", "observe_packed", "begin", "delays", "state", "load_state"):
        assert callable(getattr(P.Perturbation, method))
    for method in ("step_tensor", "reset", "step", "snapshot", "restore"):
        assert callable(getattr(P.DevicePerturbedVecEnv, method))
    for name, value in (("QG_PERTURB_DONE_ROW_RESET", _abi.PERTURB_DONE_ROW_RESET), ("QG_PERTURB_DONE_ROW_TERMINAL", _abi.PERTURB_DONE_ROW_TERMINAL),
                        ("QG_PERTURB_DONE_U8", _abi.PERTURB_DONE_U8), ("QG_PERTURB_DONE_F32", _abi.PERTURB_DONE_F32),
                        ("QG_PERTURB_MAX_DELAY", _abi.PERTURB_MAX_DELAY)):
        assert header_define(header, name) == value                     # (QG_PERTURB_DONE_* are aliases of QG_DONE_*)
    assert "qg_perturb" in open(os.path.join(ROOT, "quadruped-gym_amd", "csrc", "Makefile")).read()


def test_null_handles_are_refused():
    lib = _abi.load_library()
    buf = (C.c_float * 64)()
    assert lib.qg_perturb_destroy(None) == 0                 # as every destroy of the library
    assert lib.qg_perturb_actions_device(None, 4, buf, buf, None) == QG_ERR_ARG
    assert lib.qg_perturb_observe_device(None, 4, buf, 4, buf, 4, None, 0, None, 0, 1, None) == QG_ERR_ARG
    assert lib.qg_perturb_begin_device(None, 4, None, None, 0, None) == QG_ERR_ARG
    assert lib.qg_perturb_get_delays(None, buf) == QG_ERR_ARG
    assert lib.qg_perturb_get_state(None, buf, buf, buf) == QG_ERR_ARG
    assert lib.qg_perturb_set_state(None, buf, buf, buf) == QG_ERR_ARG
    assert lib.qg_last_error()


def _create(desc):
    lib = _abi.load_library()
    h = C.c_void_p()
    rc = lib.qg_perturb_create(0, C.byref(desc) if desc is not None else None, C.byref(h))
    if rc == 0:
        lib.qg_perturb_destroy(h)
    return rc, lib.qg_last_error().decode()


def test_bad_descriptors_are_refused_before_any_device_call():
    make = _abi.QgPerturbDesc.make
    lib = _abi.load_library()
    assert lib.qg_perturb_create(0, C.byref(make(4, 4)), None) == QG_ERR_ARG
    assert _create(None)[0] == QG_ERR_ARG
    bad = {
        "struct_size": lambda d: setattr(d, "struct_size", d.struct_size - 4),
        "n_envs": lambda d: setattr(d, "n_envs", 0),
        "n_envs outside": lambda d: setattr(d, "n_envs", 2 ** 31 - 1),
        "frame_dim": lambda d: setattr(d, "frame_dim", 65),
        "frame_dim 0": lambda d: setattr(d, "frame_dim", 0),
        "window": lambda d: setattr(d, "window", 0),
        "max_delay": lambda d: setattr(d, "max_delay", 17),
        "delays (-1": lambda d: setattr(d, "delay_lo", -1),
        "delays (3, 2)": lambda d: (setattr(d, "delay_lo", 3), setattr(d, "delay_hi", 2)),
        "delays (0, 4)": lambda d: setattr(d, "delay_hi", 4),
        "done_row": lambda d: setattr(d, "done_row", 2),
        "reserved": lambda d: setattr(d, "reserved", 1),
        "action_std": lambda d: setattr(d, "action_std", -0.1),
        "action_std nan": lambda d: setattr(d, "action_std", math.nan),
        "column 63": lambda d: d.obs_std.__setitem__(63, math.inf),
        "column 2": lambda d: d.bias_std.__setitem__(2, -1.0),
        "column 0": lambda d: d.bias_std.__setitem__(0, math.nan),
        "reset_action[11]": lambda d: d.reset_action.__setitem__(11, math.inf),
    }
    for word, spoil in bad.items():
        d = make(8, 26, window=3, max_delay=3, delays=(0, 3), action_std=0.1, obs_std=[0.01] * 26, bias_std=[0.02] * 26)
        spoil(d)
        rc, msg = _create(d)
        assert rc == QG_ERR_ARG and word.split()[0] in msg, (word, rc, msg)
    # a good one gets as far as the device check: QG_OK with a GPU, QG_ERR_DEVICE (-2) without
    rc, _ = _create(make(8, 26, window=3, max_delay=3, delays=(0, 3)))
    assert rc in (0, -2)


def test_mirror_has_the_c_layout(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler to build the sizeof probe with")
    D = _abi.QgPerturbDesc
    fields = [f for f, _ in D._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "quadgym.h"\nint main(void) {\n    printf("%zu", sizeof(qg_perturb_desc));\n'
                   + "".join(f'    printf(" %zu", offsetof(qg_perturb_desc, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(s) for s in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(D)] + [getattr(D, f).offset for f in fields]
    assert got[0] == 616 and D.make(4, 4).struct_size == 616
    d = D.make(7, 26, window=10, max_delay=5, delays=(1, 4), action_std=0.25, obs_std=[0.5, 0.0, 1.5], bias_std=[0.0] * 25 + [2.0],
               done_row=_abi.PERTURB_DONE_ROW_TERMINAL, seed=-1, env_index_base=32)
    assert (d.n_envs, d.frame_dim, d.window, d.max_delay, d.delay_lo, d.delay_hi, d.done_row, d.reserved) == (7, 26, 10, 5, 1, 4, 1, 0)
    assert (d.obs_std[0], d.obs_std[2], d.obs_std[3], d.bias_std[25], d.action_std) == (0.5, 1.5, 0.0, 2.0, 0.25)
    assert list(d.reset_action) == [0.0, 0.0, -0.5] * 4 == list(_abi.default_task().default_ctrl)
    assert (d.seed, d.env_index_base) == (2 ** 64 - 1, 32)


def test_column_groups_by_name():
    po = P.column_stds({"gyro": 0.01, "accel": 0.02, "euler": 0.03, "body_vel": [0.1, 0.2]}, 26)
    assert po[:11].tolist() == pytest.approx([0.01] * 3 + [0.02] * 3 + [0.03] * 3 + [0.1, 0.2]) and not po[11:].any()
    full = P.column_stds({"accel": 0.01, "gyro": 0.01, "body_vel": 0.01}, 33)
    assert [c for c in range(33) if full[c]] == list(range(12, 18)) + [30, 31, 32]
    imu = P.column_stds({"accel": 0.01, "gyro": 0.01, "body_vel": 0.01}, 21)
    assert [c for c in range(21) if imu[c]] == list(range(12, 21))
    assert P.column_stds(None, 5).tolist() == [0.0] * 5 and P.column_stds(0.5, 3).tolist() == [0.5] * 3
    with pytest.raises(ValueError):
        P.column_stds({"euler": 0.1}, 33)
    with pytest.raises(ValueError):
        P.column_stds({"gyro": 0.1}, 7)
    with pytest.raises(ValueError):
        P.column_stds([0.1, 0.2], 3)
