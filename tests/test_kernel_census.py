"""The leaf matrix is complete (no GPU): every step-kernel instantiation the launch sites of the step-kernel units can produce has a row in
tests/kernel_leaves.py -- an oracle case in tests/test_kernel_leaves_gpu.py, or a bit-identical twin case in tests/test_resident_gpu.py
for the many-env-steps forms -- and the tables list nothing the source cannot launch."""
import os
import re

import pytest

import kernel_leaves as K


@pytest.fixture(scope="module")
def src():
    return "\n".join(open(p).read() for p in K.STEP_UNITS)


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
    # a leaf added to a selector without a row is caught
    body_end = src.index("static void select_step_quad(")
    extra = src[:body_end] + src[body_end:].replace("\n}\n", "\n    launch_quad<2, true, false, 1>(L);\n}\n", 1)
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


def test_step_shell_exists_once():
    """The shell of an env-step (state load / store, reward, terminations, auto-reset, tile copy-out) is text of qg_step_shell.h that the
    step kernels expand, not a copy per kernel: each fragment occurs once in the .hip / .h / .inc files of csrc/.  A copy that stays
    for the listing's sake (tools/asm_diff.py) is named here with its reason, and the count is what the tree has."""
    csrc = K.CSRC
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".inc"))}
    assert "qg_step_shell.h" in text

    def sites(needle):
        return [(f, ln) for f, t in text.items() for ln in t.split("\n") if needle in ln]

    def files(needle):
        return [f for f, _ in sites(needle)]

    shell = ["qg_step_shell.h"]
    # the random heading draw of the auto-reset and of qg_reset_kernel
    assert files("6.283185307179586f * uniform24(") == shell
    # the plain reward: one call site besides the definition
    assert [f for f, ln in sites("reward_total(") if "DEV float reward_total(" not in ln] == shell
    # the store of the base quaternion: once, through the access pair handed to QG_BASE_STORE (plain or byte-offset form) ...
    assert files("PUT(ST.qpos, 3, n, e, B.qw)") == shell
    assert files("lk_st(P.st.qpos, 3 * n4") == []
    # ... and the one place that spells the plain index out is not a copy of it: qg_reset_kernel has no BaseState and hands
    # st.qpos[3 * n + env] .. [6 * n + env] to QG_RESET_HEADING as the heading's destination
    assert files(".qpos[3 * n") == ["qg_capi.hip"]
    assert all("QG_RESET_HEADING(" in ln for _, ln in sites(".qpos[3 * n"))
    # the bad-state termination: the shell's, and the one-env-per-lane kernel's own (it adds the base first and its 24 hinge values
    # one by one from LDS -- another order of the additions, so another rounding: not the shell's probe)
    assert files("state_is_bad(probe)") == ["qg_kernel_quad.hip", "qg_step_shell.h"]
    # tile copy-out multipliers, model staging, task snapshot, reward components
    for needle in ("const unsigned magic =", "reinterpret_cast<float *>(&smodel)", "Tk = {T->frame_skip", "P.comps[(size_t)env * 3 + 0]"):
        assert files(needle) == shell, needle
    # hinge state: through QG_HINGE_LOAD / QG_HINGE_STORE, except in the one-link-per-lane kernels -- per-launch and many-steps form,
    # a load and a store each -- whose listings change with the macros' (7 + j) * n4 + e4 for their 7 * n4 + (j * n4 + e4)
    assert files("P.st.qpos[(7 + j) * n") == []
    assert files("7 * n4 + j4") == ["qg_kernel_link.hip"] * 2 + ["qg_kernel_resident.hip"] * 2


def test_rows_shell_exists_once():
    """The shell of a rows kernel of the policy's backward passes (observation tile staged, hidden layers forward with their record
    stores, output product, walk back over the transposed image) is text of qg_policy_grad_dev.h that both rows kernels expand around
    their own heads, not a copy per kernel: each characteristic line occurs once in the .hip / .h / .inc files of csrc/."""
    csrc = K.CSRC
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".inc"))}
    shell = ["qg_policy_grad_dev.h"]

    def files(needle):
        return [f for f, t in text.items() for ln in t.split("\n") if needle in ln]

    for needle in (
            # the tanh-and-derivative loop of a hidden layer
            "const double t = tanh(sum[r]);", "dh[r] = (float)(1.0 - t * t);",
            # the W^T delta product of the walk back, and the delta it forms
            "qgg_product(packed_t + GL.wt_off, L.nb, m, din, sum, lane);", "d[r] = (float)(sum[r] * (double)dh[r]);",
            # the record stores: the staged observation, a hidden layer's h and tanh', the output delta, the delta of the walk back
            "rec[(size_t)(row0 + ee) * G.rec + G.layer[tower][0].h_off + c] = v;", "(myrec + h_next + 16 * m + 4 * g) = h;",
            "(myrec + d_own + 16 * m + 4 * g) = dh;", "(myrec + G.layer[tower][l].d_off + 4 * g) = D", "(myrec + d_prev + 16 * m + 4 * g) = d;"):
        assert files(needle) == shell, needle
    # both rows kernels expand every piece of it, once, in their bodies
    pieces = ["QGG_ROWS_ENTRY(", "QGG_ROWS_STAGE(", "QGG_ROWS_LAYER(", "QGG_ROWS_HIDDEN(", "QGG_ROWS_OUTPUT(", "QGG_ROWS_DELTA(", "QGG_ROWS_WALK_BACK("]
    for unit, kernel in (("qg_policy_grad.hip", "qg_policy_grad_rows_kernel"), ("qg_policy_distill.hip", "qg_policy_distill_rows_kernel")):
        body = text[unit].split("void %s(" % kernel, 1)[1].split("\n}\n", 1)[0]
        assert [body.count(p) for p in pieces] == [1] * len(pieces), unit
        assert [text[unit].count(p) for p in pieces] == [1] * len(pieces), unit
    assert all(text["qg_policy_grad_dev.h"].count("#define " + p) == 1 for p in pieces)
    # the two row sums stay two (the butterfly and the ascending order round differently), both beside the shell
    assert files("double qgg_sum_rows(double v)") == shell and files("double qgd_sum_rows(double v, int lane)") == shell
