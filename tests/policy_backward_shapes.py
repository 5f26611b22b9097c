"""The geometry of the fused policy's backward passes and optimiser step, restated from a description ``(obs_dim, hidden, act_dim)``
and a critic flag alone -- from DESIGN 4.11 / 4.13 / 4.19 and the comments of csrc/qg_policy.h, not from the kernels' text -- and the
shape classes a description meets in them.  The census of tests/test_policy_backward_census.py is taken with it, and the cases of
tests/test_policy_backward_shapes_gpu.py (every row of policy_reference.SHAPE_TABLE) are listed here so that the CPU census and the GPU
module see the same data.  NumPy only; nothing here touches the GPU.

The geometry.  A layer ``in_dim -> out_dim`` has ``nq = ceil(in_dim / 16)`` input blocks and ``nb = ceil(out_dim / 16)`` output blocks.
* rows kernels (PPO and distillation): a product runs over ``nk`` operand blocks in groups of GROUP = 4, the last group clamped and
  guarded (``nk % 4``); forward ``nk = nq``; a hidden layer's ``nb`` blocks go round WAVES = 4 waves; the walk back through layer
  ``l >= 1`` is the product with ``nk = nb`` for each of the ``nq`` blocks of the layer's input, again round the four waves.  The heads
  hold action ``a`` in quarter ``a // 4`` (lanes ``g = lane >> 4``), element ``a % 4``.
* weights launch: a work item is up to ITEM_BLOCKS = 4 consecutive output blocks (an m-group) times one input block, ``ceil(nb / 4) x
  nq`` items per layer, layers in tower-major order, and one final item for the tiles' scalars.
* Adam: the canonical vector ``W, b, .., log_std, critic W, b, ..`` is cut into ADAM_SLOT elements per workgroup and ADAM_GROUP = 4
  consecutive elements per thread; a thread carries the region (and in a W the row and column) from one element of its group to the
  next, so what matters is where a region boundary falls inside a group (``boundary % 4``) and whether a W's row ends inside one."""
import collections
import functools
import itertools

import numpy as np

import distill_reference as D
import policy_reference as R
import ppo_reference as G

WAVES, GROUP, ITEM_BLOCKS = 4, 4, 4
ADAM_SLOT, ADAM_GROUP = 2048, 4

Layer = collections.namedtuple("Layer", ["tower", "index", "in_dim", "out_dim", "nq", "nb"])
Region = collections.namedtuple("Region", ["name", "kind", "lo", "hi", "in_dim"])       # kind: W, b, log_std; in_dim of a W, else 0


def _blocks(width):
    return -(-width // 16)


def layers(desc, critic):
    """Tower-major (the actor, then the critic): the order of the canonical vector, of the row record and of the work items."""
    obs_dim, hidden, act_dim = desc
    out = []
    for tower, last in (("actor", act_dim), ("critic", 1))[:2 if critic else 1]:
        dims = (obs_dim,) + tuple(hidden) + (last,)
        out += [Layer(tower, k, dims[k], dims[k + 1], _blocks(dims[k]), _blocks(dims[k + 1])) for k in range(len(dims) - 1)]
    return out


def work_items(desc, critic):
    """``([items per layer, tower-major], total)``; the total counts the final scalar item."""
    per = [-(-L.nb // ITEM_BLOCKS) * L.nq for L in layers(desc, critic)]
    return per, sum(per) + 1


def regions(desc, critic):
    """The canonical regions in order, named as FusedMlpPolicy.param_layout names them."""
    out, off = [], 0
    for L in layers(desc, critic):
        if L.tower == "critic" and L.index == 0:
            out.append(Region("log_std", "log_std", off, off + desc[2], 0))
            off += desc[2]
        out.append(Region(f"{L.tower}.{L.index}.weight", "W", off, off + L.out_dim * L.in_dim, L.in_dim))
        off += L.out_dim * L.in_dim
        out.append(Region(f"{L.tower}.{L.index}.bias", "b", off, off + L.out_dim, 0))
        off += L.out_dim
    if not critic:
        out.append(Region("log_std", "log_std", off, off + desc[2], 0))
    return out


def n_params(desc, critic):
    return regions(desc, critic)[-1].hi


# ---- the classes ----------------------------------------------------------------------------------------------------------------------
BOUNDARY_KINDS = ("W->b", "b->W", "b->log_std", "log_std->critic W", "log_std->end", "critic b->end")


def _product(prefix, nk):
    groups = -(-nk // GROUP)
    return {f"{prefix}:nk%4={nk % GROUP}", f"{prefix}:groups={groups if groups < 3 else '>=3'}"}


def _waves(prefix, count):
    if count < WAVES:
        return f"{prefix}<4"
    if count == WAVES:
        return f"{prefix}=4"
    return f"{prefix}>4,ragged" if count % WAVES else f"{prefix}>4,multiple"


def boundaries(desc, critic):
    """``[(kind, offset)]`` of every region boundary of the canonical vector, its end included."""
    regs, out = regions(desc, critic), []
    for a, b in zip(regs, regs[1:] + [None]):
        if b is None:
            kind = "critic b->end" if critic else "log_std->end"
        elif a.kind == "W":
            kind = "W->b"
        elif a.kind == "b":
            kind = "b->log_std" if b.kind == "log_std" else "b->W"
        else:
            kind = "log_std->critic W"
        out.append((kind, a.hi))
    return out


def backward_classes(desc, critic):
    """The classes of the rows kernels and the weights launch that ``desc`` meets (the PPO pass with both towers when ``critic``)."""
    obs_dim, hidden, act_dim = desc
    names = set()
    for L in layers(desc, critic):
        names |= _product("fwd", L.nq)
        if L.nq == 32:
            names.add("fwd:nk=32")
        if L.index < len(hidden):
            names.add(_waves("hidden:nb", L.nb))
        if L.index >= 1:
            names |= _product("back", L.nb)
            names.add(_waves("back:nq", L.nq))
        mgroups = -(-L.nb // ITEM_BLOCKS)
        names |= {f"weights:last-m-group={L.nb - ITEM_BLOCKS * (mgroups - 1)}", f"weights:m-groups={mgroups if mgroups < 3 else '>=3'}",
                  "weights:in-padded" if L.in_dim % 16 else "weights:in-exact", "weights:out-padded" if L.out_dim % 16 else "weights:out-exact"}
        if L.in_dim == 1:
            names.add("weights:in=1")
    if critic:
        names.add("weights:two-towers")
    names |= {f"head:quarter={(act_dim - 1) // 4}", f"head:act%4={act_dim % 4}", f"head:hidden={len(hidden)}"}
    if act_dim in (1, 16):
        names.add(f"head:act={act_dim}")
    return names


def update_classes(desc, critic):
    """What the Adam step's elementwise part meets, whatever happens to the images: the ragged tail of the last group of four."""
    return {f"adam:tail={n_params(desc, critic) % ADAM_GROUP}"}


def scatter_classes(desc, critic, transposed):
    """What the Adam step's scatter into the operand images meets."""
    names = {f"scatter:{kind}@{off % ADAM_GROUP}" for kind, off in boundaries(desc, critic)}
    if any(r.kind == "W" and r.in_dim < ADAM_GROUP for r in regions(desc, critic)):
        names.add("scatter:in<4")
    names.add("scatter:transposed" if transposed else "scatter:forward-only")
    return names


@functools.lru_cache(maxsize=None)
def reachable_alignments():
    """``{kind: set of boundary % 4}`` over the descriptions the ABI accepts, by enumeration: every ``obs_dim`` residue, every width
    alone and three widths in every arrangement of up to three layers, every ``act_dim``, with and without a critic.  (Why the result
    is what it is: hidden widths are multiples of 16, so every W and every hidden b is a multiple of 16 long; the only odd lengths are
    the actor's last bias and ``log_std`` (``act_dim`` each) and the critic's last bias (1).  The actor's own boundaries sit at 0,
    ``b -> log_std`` at ``act_dim % 4``, everything from ``log_std``'s end to the critic's last W at ``2 act_dim % 4``, the end of a
    vector with a critic one past that.)"""
    widths = tuple(range(16, 257, 16))
    hiddens = [(w,) for w in widths] + [h for n in (2, 3) for h in itertools.product((16, 48, 256), repeat=n)]
    out = {kind: set() for kind in BOUNDARY_KINDS}
    for obs_dim in list(range(1, 17)) + [511, 512]:
        for hidden in hiddens:
            for act_dim in range(1, 17):
                for critic in (False, True):
                    for kind, off in boundaries((obs_dim, hidden, act_dim), critic):
                        out[kind].add(off % ADAM_GROUP)
    return out


def required_backward():
    """Every class of the rows kernels and the weights launch, written out."""
    names = {f"{p}:nk%4={r}" for p in ("fwd", "back") for r in range(4)} | {f"{p}:groups={g}" for p in ("fwd", "back") for g in (1, 2, ">=3")}
    names |= {"fwd:nk=32"} | {f"{p}{c}" for p in ("hidden:nb", "back:nq") for c in ("<4", "=4", ">4,ragged", ">4,multiple")}
    names |= {f"head:quarter={k}" for k in range(4)} | {f"head:act%4={r}" for r in range(4)} | {"head:act=1", "head:act=16"}
    names |= {f"head:hidden={n}" for n in (1, 2, 3)}
    names |= {f"weights:last-m-group={s}" for s in (1, 2, 3, 4)} | {f"weights:m-groups={g}" for g in (1, 2, ">=3")}
    names |= {"weights:in-padded", "weights:in-exact", "weights:out-padded", "weights:out-exact", "weights:in=1", "weights:two-towers"}
    return names


def required_scatter():
    names = {f"scatter:{kind}@{a}" for kind, aligns in reachable_alignments().items() for a in aligns}
    return names | {"scatter:in<4", "scatter:transposed", "scatter:forward-only"}


def required_update():
    return {f"adam:tail={r}" for r in range(4)}


def census(nets, critics=(False, True), transposed=(False, True)):
    """``(backward, scatter, update)``: the classes a collection of descriptions meets; ``nets`` holds ``(obs_dim, hidden, act_dim)``,
    taken with each of ``critics``, or ``(obs_dim, hidden, act_dim, critic)``."""
    back, scat, upd = set(), set(), set()
    for net in nets:
        for critic in (critics if len(net) == 3 else (net[3],)):
            back |= backward_classes(net[:3], critic)
            upd |= update_classes(net[:3], critic)
            for tr in transposed:
                scat |= scatter_classes(net[:3], critic, tr)
    return back, scat, upd


# ---- the cases of tests/test_policy_backward_shapes_gpu.py ----------------------------------------------------------------------------
TABLE = range(len(R.SHAPE_TABLE))
B_SMALL, B_TWO_SLOTS = 83, G.SLOT_ROWS + 1            # five tiles and a three-row tail; two slots


def row_id(i):
    obs_dim, hidden, act_dim = R.SHAPE_TABLE[i]
    return "%d-%s-%d" % (obs_dim, "-".join(str(h) for h in hidden), act_dim)


def out_tanh(i):
    return bool(i % 2)


def clip_range_vf(i):
    return 0.3 if (i // 2) % 2 else None


# the rows that carry act_dim >= 13 (head lanes g == 3, misc[12..15]) or nk == 32: these also run at two slots
CARRIERS = tuple(i for i in TABLE if R.SHAPE_TABLE[i][2] >= 13 or _blocks(R.SHAPE_TABLE[i][0]) == 32)
# ... where g == 3 is live in every element or all but one: the placement cases
PLACEMENT_ROWS = tuple(i for i in TABLE if R.SHAPE_TABLE[i][2] >= 15)
POSITIONS = (0, 15, 16, 82)


def ppo_cases():
    """``ppo_reference.Case``s: every row at 83 rows with a critic, rows ``i % 3 == 0`` also without, the carriers also at 513."""
    cases = []
    for i in TABLE:
        for B in (B_SMALL,) + ((B_TWO_SLOTS,) if i in CARRIERS else ()):
            for value in (True,) + ((False,) if i % 3 == 0 and B == B_SMALL else ()):
                cases.append(G.Case(R.SHAPE_TABLE[i], B, out_tanh(i), clip_range_vf(i), value, 7000 + 10 * i + (B > 100)))
    return cases


@functools.lru_cache(maxsize=None)
def build_ppo_case(case):
    """``ppo_reference.build_case``, made once and read-only."""
    actor, log_std, critic, batch = G.build_case(case)
    for a in [log_std] + [x for W, b in actor + (critic or []) for x in (W, b)] + [x for x in batch if x is not None]:
        a.setflags(write=False)
    return actor, log_std, critic, batch


DistillCase = collections.namedtuple("DistillCase", ["i", "B", "mode", "weights"])


def distill_cases():
    """Mode and kind of weights rotate along the table (the mode with ``(i // 2) % 2``, against ``out_tanh``'s ``i % 2``; the weights
    with ``i % 3``); the rows with ``act_dim >= 13`` or ``act_dim == 1`` run both modes with all three kinds; the carriers run at 513
    rows too, in both modes."""
    cases = []
    for i in TABLE:
        act_dim = R.SHAPE_TABLE[i][2]
        mode, kind = D.MODES[(i // 2) % 2], D.WEIGHTS[i % 3]
        if act_dim >= 13 or act_dim == 1:
            cases += [DistillCase(i, B_SMALL, m, k) for m in D.MODES for k in D.WEIGHTS]
        else:
            cases.append(DistillCase(i, B_SMALL, mode, kind))
        if i in CARRIERS:
            cases += [DistillCase(i, B_TWO_SLOTS, m, D.WEIGHTS[(i + j) % 3]) for j, m in enumerate(D.MODES)]
    return cases


def distill_id(case):
    return "%s-B%d-%s-w%s" % (row_id(case.i), case.B, case.mode, case.weights)


@functools.lru_cache(maxsize=None)
def distill_data(i, B):
    """``distill_reference.make_data`` of row ``i`` (with a critic, no weights), seeded per row and size, read-only."""
    data = D.make_data(np.random.default_rng(8000 + 10 * i + (B > 100)), R.SHAPE_TABLE[i], B, out_tanh(i), True)
    for a in [data.log_std, data.obs, data.target, data.target_log_std] + [x for W, b in data.actor + data.critic for x in (W, b)]:
        a.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def distill_weights(i, B, kind):
    """``distill_reference.make_weights`` (kind ``zeros`` keeps row 0 live), seeded per row, size and kind."""
    w = D.make_weights(np.random.default_rng([8500 + 10 * i + (B > 100), D.WEIGHTS.index(kind)]), B, kind)
    if w is not None:
        w.setflags(write=False)
    return w


def distill_kwargs(case, coef=0.7):
    data = distill_data(case.i, case.B)
    return dict(out_tanh=out_tanh(case.i), mode=case.mode, coef=coef, target_log_std=data.target_log_std if case.mode == "kl" else None,
                weights=distill_weights(case.i, case.B, case.weights))


# ---- the Adam step ---------------------------------------------------------------------------------------------------------------------
def adam_desc(i, critic):
    """Row ``i`` as a description of tests/adam_reference.py: ``(obs_dim, hidden, act_dim, critic)``."""
    return R.SHAPE_TABLE[i] + (bool(critic),)


def adam_float64_rows(old_nets):
    """The ``(i, critic)`` that carry a tail ``n_params % 4`` or a boundary alignment none of ``old_nets`` has: for each such class the
    first row of the table that meets it."""
    _, old_scatter, old_update = census(old_nets)
    rows = []
    for name in sorted((required_update() - old_update) | {c for c in required_scatter() - old_scatter if "@" in c}):
        found = next((i, critic) for i in TABLE for critic in (False, True)
                     if name in update_classes(R.SHAPE_TABLE[i], critic) | scatter_classes(R.SHAPE_TABLE[i], critic, True))
        if found not in rows:
            rows.append(found)
    return sorted(rows)
