"""The leaf matrix is complete (no GPU): every step-kernel instantiation the launch sites of qg_capi.hip can produce has a row in
tests/kernel_leaves.py -- an oracle case in tests/test_kernel_leaves_gpu.py, or a bit-identical twin case in tests/test_resident_gpu.py
for the many-env-steps forms -- and the tables list nothing the source cannot launch."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_leaves as K  # noqa: E402


@pytest.fixture(scope="module")
def src():
    return open(K.CAPI).read()


def test_launch_sites_equal_the_matrix(src):
    launched = K.launched_instantiations(src)
    tables = set(K.LEAVES) | set(K.MULTI_TWINS)
    assert launched - tables == set(), "step kernels with no oracle case in tests/kernel_leaves.py"
    assert tables - launched == set(), "rows for step kernels no launch site produces"
    assert len(K.LEAVES) == 38 and len(K.MULTI_TWINS) == 9


def test_census_parses_defaults_and_dyn(src):
    params = K.launcher_parameters(src)
    assert [p for p, _ in params["quad"]] == ["WPE", "BAKED", "WALK", "WAVES", "PO", "HELP", "DYN"]
    assert [d for _, d in params["quad"]][4:] == [0, 0, 0]
    assert set(params) == {"lane", "link", "quad", "pair", "link_multi", "quad_multi", "pair_multi"}
    # a leaf added to select_step without a row is caught
    body_end = src.index("static void select_step(")
    extra = src[:body_end] + src[body_end:].replace("        break;\n", "        launch_quad<2, true, false, 1>(L);\n        break;\n", 1)
    assert K.launched_instantiations(extra) - set(K.LEAVES) - set(K.MULTI_TWINS) == {"qg_step_kernel_quad<2,1,0,1,0,0,0>"}


def test_twin_cases_exist():
    """Every multi-step form names a test_resident_gpu.py case (and parameter id) that exists, and a leaf of the oracle matrix."""
    text = open(os.path.join(K.ROOT, "tests", "test_resident_gpu.py")).read()
    for multi, (case, leaf) in K.MULTI_TWINS.items():
        assert leaf in K.LEAVES, multi
        func = case.split("::")[1].split("[")[0]
        assert re.search(r"^def %s\(" % func, text, re.M), case
        if "[" in case:
            ident = case.split("[")[1].rstrip("]")
            assert "(%s)" % ident.replace("-", ", ") in text, case


def test_last_step_kernel_is_declared():
    header = open(os.path.join(K.ROOT, "include", "quadgym.h")).read()
    assert re.search(r"int32_t qg_debug_last_step_kernel\(const qg_sim \*sim, char \*buf, int32_t len\);", header)
