"""The optimiser step and the advantage normaliser without a GPU: the five entry points exist in the library, the header and the
binding; NULL handles are refused before any device check; the ctypes mirror of qg_adam_params has the C size; the slot constant the GPU
tests take their shapes from is the kernel's."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from quadruped_gym_amd import _abi
from quadruped_gym_amd.policy import FusedMlpPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QG_ERR_ARG = -1
NEW = ("qg_policy_reserve_adam", "qg_policy_adam_update_device", "qg_policy_adam_get_state", "qg_policy_adam_set_state",
       "qg_policy_normalize_advantages_device")


def test_symbols_are_exported_declared_and_bound():
    lib = _abi.load_library()
    header = open(os.path.join(ROOT, "include", "quadgym.h")).read()
    for name in NEW:
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"int {name}(" in header
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    for word in ("typedef struct qg_adam_params", "TWO launches", "ONE launch"):
        assert word in header
    for method in ("reserve_adam", "adam_step", "adam_state", "load_adam_state", "normalize_advantages"):
        assert callable(getattr(FusedMlpPolicy, method))


def test_null_handles_are_refused():
    lib = _abi.load_library()
    buf, step = (C.c_float * 8)(), C.c_int64()
    params = _abi.QgAdamParams.make()
    assert lib.qg_policy_reserve_adam(None) == QG_ERR_ARG
    assert lib.qg_policy_adam_update_device(None, C.byref(params), buf, None, None, None, None) == QG_ERR_ARG
    assert lib.qg_policy_adam_get_state(None, buf, buf, C.byref(step)) == QG_ERR_ARG
    assert lib.qg_policy_adam_set_state(None, buf, buf, 0) == QG_ERR_ARG
    assert lib.qg_policy_normalize_advantages_device(None, 8, buf, buf, None) == QG_ERR_ARG
    assert lib.qg_last_error()


def test_mirror_has_the_c_size(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler to build the sizeof probe with")
    src = tmp_path / "probe.c"
    fields = [f for f, _ in _abi.QgAdamParams._fields_]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "quadgym.h"\nint main(void) {\n    printf("%zu", sizeof(qg_adam_params));\n'
                   + "".join(f'    printf(" %zu", offsetof(qg_adam_params, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(s) for s in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_abi.QgAdamParams)] + [getattr(_abi.QgAdamParams, f).offset for f in fields]
    assert got[0] == 28 and _abi.QgAdamParams.make().struct_size == 28
    d = _abi.QgAdamParams.make(1e-3, (0.8, 0.99), 1e-5, None)
    assert (d.reserved, d.max_grad_norm) == (0, 0.0) and abs(d.lr - 1e-3) < 1e-9 and abs(d.beta_two - 0.99) < 1e-7 and abs(d.eps - 1e-5) < 1e-12


def test_slot_constant_agrees_with_the_kernel():
    text = open(os.path.join(ROOT, "quadruped-gym_amd", "csrc", "qg_policy.h")).read()
    slot = int(re.search(r"#define QGA_SLOT (\d+)", text).group(1))
    threads = int(re.search(r"#define QGA_THREADS (\d+)", text).group(1))
    assert FusedMlpPolicy.ADAM_SLOT == slot and slot % (4 * threads) == 0
