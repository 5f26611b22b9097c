"""The census of the fused policy's backward passes and optimiser step, without a GPU: which shape classes of the rows kernels, the
weights launch and the Adam scatter (tests/policy_backward_shapes.py) the rows of policy_reference.SHAPE_TABLE meet -- every one --,
and which of them the nets those kernels were tested on before met -- not all.

The gap this module pins (tests/test_policy_backward_shapes_gpu.py closes it by running every row of the table):
* ``ppo_grad`` and ``distill_grad`` ran on ppo_reference.NETS + WIDE, whose ``act_dim`` is 1, 4, 7 or 12 and whose ``obs_dim`` is 3 to
  260.  They miss: the fourth head quarter (``head:quarter=3``, actions 12..15: the lanes ``g == 3`` of the heads, the ``misc[12..15]``
  sums, rows 12..15 of the output layer's dW and db), ``head:act=16`` (no padding in the output block), ``head:act%4=2``,
  ``fwd:nk=32`` (``obs_dim`` 497..512: eight operand groups, the largest record) and ``weights:in=1`` (a one-column first layer).
* ``adam_step``'s images were compared with what ``set_params`` packs on adam_reference's nets B and C alone (the asymmetric-critic
  and distillation modules use ``act_dim`` 12 too): both have ``act_dim`` 12 and a critic, so every region boundary falls on a
  multiple of four and no thread's group of four elements ever crosses one.  They miss every boundary at an alignment other than 0,
  ``critic b->end`` at 3, the vector that ends with ``log_std`` (no critic) at either alignment, and ``scatter:in<4`` (a W whose rows
  end inside a group: the row carry).
* the step itself (p, m, v) ran on nets A, B and C, whose ``n_params % 4`` is 2, 1, 1: the tails 0 and 3 are missed.
A narrower table, or a wider old set, fails here until the lists below are brought up to date."""
import os
import re

import numpy as np
import pytest

import adam_reference as A
import policy_backward_shapes as S
import policy_reference as R
import ppo_reference as G

from quadruped_gym_amd.policy import FusedMlpPolicy

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quadruped-gym_amd", "csrc")

# written out: what the table must meet
BACKWARD = {
    "fwd:nk%4=0", "fwd:nk%4=1", "fwd:nk%4=2", "fwd:nk%4=3", "fwd:groups=1", "fwd:groups=2", "fwd:groups=>=3", "fwd:nk=32",
    "hidden:nb<4", "hidden:nb=4", "hidden:nb>4,ragged", "hidden:nb>4,multiple",
    "back:nk%4=0", "back:nk%4=1", "back:nk%4=2", "back:nk%4=3", "back:groups=1", "back:groups=2", "back:groups=>=3",
    "back:nq<4", "back:nq=4", "back:nq>4,ragged", "back:nq>4,multiple",
    "head:quarter=0", "head:quarter=1", "head:quarter=2", "head:quarter=3", "head:act%4=0", "head:act%4=1", "head:act%4=2", "head:act%4=3",
    "head:act=1", "head:act=16", "head:hidden=1", "head:hidden=2", "head:hidden=3",
    "weights:last-m-group=1", "weights:last-m-group=2", "weights:last-m-group=3", "weights:last-m-group=4",
    "weights:m-groups=1", "weights:m-groups=2", "weights:m-groups=>=3",
    "weights:in-padded", "weights:in-exact", "weights:out-padded", "weights:out-exact", "weights:in=1", "weights:two-towers",
}
# the alignments the ABI's shapes can give each kind of boundary (policy_backward_shapes.reachable_alignments derives them)
ALIGNMENTS = {"W->b": {0, 2}, "b->W": {0, 2}, "b->log_std": {0, 1, 2, 3}, "log_std->critic W": {0, 2}, "log_std->end": {0, 2},
              "critic b->end": {1, 3}}
SCATTER = {f"scatter:{kind}@{a}" for kind, aligns in ALIGNMENTS.items() for a in aligns} | {"scatter:in<4", "scatter:transposed",
                                                                                           "scatter:forward-only"}
UPDATE = {"adam:tail=0", "adam:tail=1", "adam:tail=2", "adam:tail=3"}

# ... and what the nets of the older tests miss
OLD_BACKWARD_MISSES = {"head:quarter=3", "head:act=16", "head:act%4=2", "fwd:nk=32", "weights:in=1"}
OLD_SCATTER_MISSES = {"scatter:W->b@2", "scatter:b->W@2", "scatter:b->log_std@1", "scatter:b->log_std@2", "scatter:b->log_std@3",
                      "scatter:log_std->critic W@2", "scatter:critic b->end@3", "scatter:log_std->end@0", "scatter:log_std->end@2",
                      "scatter:in<4"}
OLD_UPDATE_MISSES = {"adam:tail=0", "adam:tail=3"}


def test_the_written_out_lists_are_the_helpers():
    assert BACKWARD == S.required_backward() and SCATTER == S.required_scatter() and UPDATE == S.required_update()
    assert S.reachable_alignments() == ALIGNMENTS and set(ALIGNMENTS) == set(S.BOUNDARY_KINDS)


@pytest.mark.parametrize("critic", [False, True])
@pytest.mark.parametrize("i", S.TABLE, ids=S.row_id)
def test_canonical_regions_equal_param_layout(i, critic):
    desc = R.SHAPE_TABLE[i]
    layout = FusedMlpPolicy.param_layout(*desc, value=critic)
    regs = S.regions(desc, critic)
    assert [(r.name, r.lo, r.hi - r.lo) for r in regs] == [(k, off, int(np.prod(shape))) for k, (off, shape) in layout.items()]
    assert all(r.in_dim == layout[r.name][1][1] for r in regs if r.kind == "W")
    assert S.n_params(desc, critic) == R.param_count(*desc, critic)
    assert [b for _, b in S.boundaries(desc, critic)] == [r.hi for r in regs]


def test_geometry_of_known_descriptions():
    """By hand.  33-64-64-12 with a critic: layers of (nq, nb) = (3, 4), (4, 4), (4, 1) per tower, 3 + 4 + 4 items each and the scalar
    item; 129-240-96-176-15: nq = 9, nb = 15: four m-groups, the last of three blocks."""
    assert [(L.nq, L.nb) for L in S.layers((33, (64, 64), 12), True)] == [(3, 4), (4, 4), (4, 1)] * 2
    assert S.work_items((33, (64, 64), 12), True) == ([3, 4, 4, 3, 4, 4], 23) and S.work_items((33, (64, 64), 12), False) == ([3, 4, 4], 12)
    first = S.layers((129, (240, 96, 176), 15), False)[0]
    assert (first.nq, first.nb) == (9, 15) and S.work_items((129, (240, 96, 176), 15), False)[0] == [36, 30, 18, 11]
    wide = S.backward_classes((129, (240, 96, 176), 15), False)
    assert {"weights:last-m-group=3", "weights:m-groups=>=3", "fwd:nk%4=1", "fwd:groups=>=3", "hidden:nb>4,ragged", "back:nk%4=2",
            "head:quarter=3", "head:act%4=3", "head:hidden=3"} <= wide and "weights:two-towers" not in wide
    # 1-16-1 with a critic: 16 + 16 + 16 + 1 + 1 = 50 elements, then the critic's 16 + 16 + 16 + 1
    assert [off for _, off in S.boundaries((1, (16,), 1), True)] == [16, 32, 48, 49, 50, 66, 82, 98, 99]
    assert S.scatter_classes((1, (16,), 1), True, False) == {"scatter:W->b@0", "scatter:b->W@0", "scatter:b->log_std@1",
                                                             "scatter:log_std->critic W@2", "scatter:W->b@2", "scatter:b->W@2",
                                                             "scatter:critic b->end@3", "scatter:in<4", "scatter:forward-only"}


def test_shape_table_meets_every_class():
    back, scat, upd = S.census(R.SHAPE_TABLE)
    assert BACKWARD - back == set() and back - BACKWARD == set()
    assert SCATTER - scat == set() and scat - SCATTER == set()
    assert upd == UPDATE


def test_the_older_nets_miss_exactly_what_the_docstring_names():
    back, _, _ = S.census(G.NETS + (G.WIDE,))
    assert BACKWARD - back == OLD_BACKWARD_MISSES
    _, scat, _ = S.census([A.NETS[k] for k in "BC"])           # the two nets whose images were compared
    assert SCATTER - scat == OLD_SCATTER_MISSES
    _, _, upd = S.census([A.NETS[k] for k in "ABC"])
    assert UPDATE - upd == OLD_UPDATE_MISSES
    assert {n[2] for n in G.NETS + (G.WIDE,)} == {1, 4, 7, 12} and {A.NETS[k][2] for k in "BC"} == {12}


def test_the_carriers_and_the_float64_rows_are_what_the_census_says():
    descs = [R.SHAPE_TABLE[i] for i in S.CARRIERS]
    assert {(63, (64, 16), 13), (129, (240, 96, 176), 15), (64, (48, 32, 16), 16), (512, (256, 256, 256), 16)} <= set(descs)
    assert all(d[2] >= 13 or "fwd:nk=32" in S.backward_classes(d, True) for d in descs)
    assert all(i in S.CARRIERS for i in S.TABLE if {"head:quarter=3", "fwd:nk=32"} & S.backward_classes(R.SHAPE_TABLE[i], True))
    assert {R.SHAPE_TABLE[i][2] for i in S.PLACEMENT_ROWS} == {15, 16}
    rows = S.adam_float64_rows([A.NETS[k] for k in "ABC"])
    _, scat, upd = S.census([S.adam_desc(i, c) for i, c in rows] + [A.NETS[k] for k in "ABC"], transposed=(True,))
    assert upd == UPDATE and {c for c in SCATTER if "@" in c} <= scat


def test_constants_agree_with_the_kernels():
    dev = open(os.path.join(CSRC, "qg_policy_grad_dev.h")).read()
    assert int(re.search(r"#define QGG_WAVES (\d+)", dev).group(1)) == S.WAVES
    group = dev[dev.index("void qgg_load_group"):dev.index("void qgg_product")]
    assert [int(x) for x in re.findall(r"for \(int u = 0; u < (\d+); u\+\+\)", group)] == [S.GROUP]
    product = dev[dev.index("void qgg_product"):dev.index("qgg_sum_rows")]
    assert [int(x) for x in re.findall(r"q0 \+= (\d+)\)", product)] == [S.GROUP] and f"q0 + {S.GROUP}, nk" in product
    assert set(re.findall(r"m \+= (\w+)\)", dev)) == {"QGG_WAVES"}
    grad = open(os.path.join(CSRC, "qg_policy_grad.hip")).read()
    m = re.search(r"item \+= \(\(L\.nb \+ (\d+)\) / (\d+)\) \* L\.nq;", grad)
    assert m and (int(m.group(1)), int(m.group(2))) == (S.ITEM_BLOCKS - 1, S.ITEM_BLOCKS)
    assert int(re.search(r"m0 = (\d+) \* \(idx / L\.nq\)", grad).group(1)) == S.ITEM_BLOCKS
    assert "g->n_items = item + 1;" in grad
    head = open(os.path.join(CSRC, "qg_policy.h")).read()
    assert int(re.search(r"#define QGA_SLOT (\d+)", head).group(1)) == S.ADAM_SLOT == FusedMlpPolicy.ADAM_SLOT
    assert int(re.search(r"#define QGP_TILE (\d+)", head).group(1)) == G.TILE_ROWS
    opt = open(os.path.join(CSRC, "qg_policy_opt.hip")).read()
    assert int(re.search(r"QGA_GROUPS = QGA_SLOT / \((\d+) \* QGA_THREADS\)", opt).group(1)) == S.ADAM_GROUP
    assert re.search(r"\(k \* QGA_THREADS \+ \(int\)threadIdx\.x\) \* (\d+)", opt).group(1) == str(S.ADAM_GROUP)
    assert (S.B_SMALL, S.B_TWO_SLOTS) == (83, FusedMlpPolicy.GRAD_SLOT_ROWS + 1)


# ---- conditions on the inputs of the GPU module's PPO cases ---------------------------------------------------------------------------
def test_case_lists():
    cases = S.ppo_cases()
    assert len(cases) == len(S.TABLE) + len([i for i in S.TABLE if i % 3 == 0]) + len(S.CARRIERS) == 39
    assert len(set(cases)) == len(cases) and {c.B for c in cases} == {83, 513}
    for i in S.TABLE:
        mine = [c for c in cases if c.net == R.SHAPE_TABLE[i]]
        assert all(c.out_tanh == bool(i % 2) and c.clip_range_vf == (0.3 if (i // 2) % 2 else None) for c in mine)
        assert {c.seed for c in mine} == {7000 + 10 * i + (c.B > 100) for c in mine}
    dist = S.distill_cases()
    for i in S.TABLE:
        mine = {(c.B, c.mode, c.weights) for c in dist if c.i == i}
        if R.SHAPE_TABLE[i][2] >= 13 or R.SHAPE_TABLE[i][2] == 1:
            assert {(83, m, k) for m in ("mse", "kl") for k in ("none", "zeros", "frac")} <= mine
        assert ({b for b, _, _ in mine} == {83, 513}) == (i in S.CARRIERS)
    assert {(c.mode, c.weights, S.out_tanh(c.i)) for c in dist} == {(m, k, t) for m in ("mse", "kl") for k in ("none", "zeros", "frac")
                                                                      for t in (False, True)}
    w = S.distill_weights(0, 83, "zeros")
    assert w[0] != 0 and 10 < np.count_nonzero(w == 0) < 50


@pytest.mark.parametrize("case", S.ppo_cases(), ids=G.case_id)
def test_every_ppo_case_has_every_class_of_row(case):
    """Conditions on the inputs, not measurements: at least 3 rows clipped high, 3 clipped low and 10 unclipped; with value clipping on,
    at least 10 rows value-clipped and 10 not; no row within BAND of a clip boundary."""
    actor, log_std, critic, batch = S.build_ppo_case(case)
    hi, lo, vc, gap = G.classes(actor, log_std, critic, batch, case.out_tanh, 0.2, case.clip_range_vf)
    n_hi, n_lo, n_vc = (int(round(f * case.B)) for f in (hi, lo, vc))
    print(f"{G.case_id(case)}: clipped high {n_hi}, low {n_lo}, value-clipped {n_vc} of {case.B}; gap {gap:.2e}")
    assert n_hi >= 3 and n_lo >= 3 and case.B - n_hi - n_lo >= 10
    if case.value and case.clip_range_vf:
        assert n_vc >= 10 and case.B - n_vc >= 10
    assert gap >= G.BAND
