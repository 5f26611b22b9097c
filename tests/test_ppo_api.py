"""The PPO loss and gradient pass without a GPU: the two entry points exist in the library, the header and the binding; argument
validation comes before the device check; FusedMlpPolicy.param_layout tiles the canonical flat vector; the ctypes mirrors of
qg_ppo_params / qg_ppo_batch have the C sizes."""
import ctypes as C
import math
import os
import shutil
import subprocess

import pytest

import policy_reference as R

from quadruped_gym_amd import _abi
from quadruped_gym_amd.policy import FusedMlpPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QG_ERR_ARG = -1
NEW = ("qg_policy_reserve_grad", "qg_policy_ppo_grad_device")


def test_symbols_are_exported_and_declared():
    lib = _abi.load_library()
    header = open(os.path.join(ROOT, "include", "quadgym.h")).read()
    for name in NEW:
        assert name in _abi.EXPORTS and hasattr(lib, name) and f"int {name}(" in header
    for word in ("typedef struct qg_ppo_params", "typedef struct qg_ppo_batch", "THREE launches"):
        assert word in header


def test_null_handles_are_refused():
    lib = _abi.load_library()
    buf = (C.c_float * 8)()
    params, batch = _abi.QgPpoParams.make(), _abi.QgPpoBatch.make(33)
    assert lib.qg_policy_reserve_grad(None, 64) == QG_ERR_ARG
    assert lib.qg_policy_ppo_grad_device(None, C.byref(params), 1, C.byref(batch), buf, buf, None) == QG_ERR_ARG
    assert lib.qg_last_error()


@pytest.mark.parametrize("value", [False, True])
@pytest.mark.parametrize("desc", [R.SHAPE_TABLE[0], R.SHAPE_TABLE[10], R.SHAPE_TABLE[20]], ids=str)
def test_param_layout_tiles_the_flat_vector(desc, value):
    obs_dim, hidden, act_dim = desc
    layout = FusedMlpPolicy.param_layout(obs_dim, hidden, act_dim, value)
    n_layers = len(hidden) + 1
    names = [f"actor.{k}.{p}" for k in range(n_layers) for p in ("weight", "bias")] + ["log_std"]
    if value:
        names += [f"critic.{k}.{p}" for k in range(n_layers) for p in ("weight", "bias")]
    assert list(layout) == names
    end = 0
    for name, (off, shape) in layout.items():
        assert off == end, name                          # in order, no gap, no overlap
        end = off + math.prod(shape)
    assert end == R.param_count(obs_dim, hidden, act_dim, value)
    d = _abi.QgPolicyDesc.make(obs_dim, hidden, act_dim, False, value)
    assert end == _abi.load_library().qg_policy_param_count(C.byref(d))
    towers = [R.tower_shapes(obs_dim, hidden, act_dim)] + ([R.tower_shapes(obs_dim, hidden, 1)] if value else [])
    for tower, shapes in zip(("actor", "critic"), towers):
        for k, (o, i) in enumerate(shapes):
            assert layout[f"{tower}.{k}.weight"][1] == (o, i) and layout[f"{tower}.{k}.bias"][1] == (o,)
    assert layout["log_std"][1] == (act_dim,)


def test_mirrors_have_the_c_sizes(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.fail("no host C compiler to build the sizeof probe with")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "quadgym.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(qg_ppo_params), sizeof(qg_ppo_batch)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sizes = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(s) for s in sizes] == [C.sizeof(_abi.QgPpoParams), C.sizeof(_abi.QgPpoBatch)] == [24, 56]
    assert _abi.QgPpoParams.make().struct_size == 24 and _abi.QgPpoBatch.make(1).struct_size == 56
    assert _abi.QgPpoParams.make(clip_range_vf=None).clip_range_vf == 0.0


def test_slot_constant_agrees_with_the_kernel():
    """FusedMlpPolicy.GRAD_SLOT_ROWS, which the GPU tests take their batch sizes from, is the kernel's QGG_SLOT_TILES x QGP_TILE."""
    text = open(os.path.join(ROOT, "quadruped-gym_amd", "csrc", "qg_policy.h")).read()
    import re
    tile = int(re.search(r"#define QGP_TILE (\d+)", text).group(1))
    slot = int(re.search(r"#define QGG_SLOT_TILES (\d+)", text).group(1))
    assert FusedMlpPolicy.GRAD_TILE_ROWS == tile and FusedMlpPolicy.GRAD_SLOT_ROWS == tile * slot
