"""Every step-kernel instantiation a handle can launch, and how a test reaches it.

``LEAVES`` holds one row per per-launch leaf of the ``select_step_*`` functions (one per mapping, in the step-kernel unit that holds the
mapping's kernels: ``STEP_UNITS``), keyed by the name
``BatchedSim.last_step_kernel`` reports: tests/test_kernel_leaves_gpu.py steps each one against the f64 oracle.  The many-env-steps
forms (``launch_*_multi``) are pinned bit for bit to a per-launch leaf by a case of tests/test_resident_gpu.py: ``MULTI_TWINS``
names that case and the leaf.  tests/test_kernel_census.py parses the launch sites and checks that both tables list exactly the
instantiations the source can launch.  ``open_leaf`` opens the handle a row describes, for every test that steps one.  Importing this
module needs neither a GPU nor torch: the product is imported where a handle is opened."""
import os
import re
from dataclasses import dataclass
from itertools import product

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quadruped-gym_amd", "csrc")
# the translation units that hold the step kernels' launch sites: one per kernel family (the census reads them joined)
STEP_UNITS = tuple(os.path.join(CSRC, f) for f in ("qg_kernel_link.hip", "qg_kernel_quad.hip", "qg_kernel_pair.hip"))

# envs per wave of each mapping (QGK_LINK_ENVS / QGK_QUAD_ENVS / QGK_PAIR_ENVS): AUTO's boundaries are "one wave per SIMD" sizes
LINK_ENVS, QUAD_ENVS, PAIR_ENVS = 4, 16, 32


def link_max(simds):            # the last size AUTO runs one link per lane (4096 on an MI355X)
    return simds * LINK_ENVS


def quad_max(simds):            # one wave of the one-leg-per-lane kernel per SIMD (16 384)
    return simds * QUAD_ENVS


def pair_max(simds):            # one wave of the two-legs-per-lane kernel per SIMD (32 768)
    return simds * PAIR_ENVS


@dataclass(frozen=True)
class Leaf:
    sizes: tuple          # functions of the device's SIMD count -> n
    robot: str = "baked"  # "baked": the compiled-in robot; "table": a slightly modified one (table-driven kernels)
    mapping: str = "auto"  # "auto" or an explicit request: "lane" / "quad" / "pair" / "link"
    layer: str = "none"   # "none" (plain step), "walk" (walking task layer fused in), "po" (and the PO observation pack)
    dyn: bool = False     # per-env dynamics rows
    helpers: bool = True  # QG_LINK_HELPERS at qg_create


PO_WINDOW = 3                 # the PO handles' obs_window in the leaf, mode-walk and rollout tests: the newest frame's place in the FIFO is part of the checks


def open_leaf(leaf, n, table=None, fs=4, auto_reset=False, reset_flags=0, seed=3, obs_window=1, **env_kw):
    """The handle `leaf` describes (its ``robot``, ``layer``, ``mapping`` and ``helpers``; a rollout_recordings.Form will do): a
    BatchedSim with the fall termination at 0.05 m for a plain step, else a walking / PO VecEnv (``env_kw`` go to it) -- (sim, env or
    None).  `table`: (path, qg_model) of the table robot (helpers.table_robot).  `auto_reset` and `reset_flags` are the plain step's
    task.  QG_LINK_HELPERS is read at qg_create: it is set for the call only."""
    from parity import MAPPINGS
    from quadruped_gym_amd import _abi
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv, WalkingQuadrupedVecEnv
    from quadruped_gym_amd.sim import BatchedSim
    path, model = table if leaf.robot == "table" else ("builtin", None)
    old = os.environ.get("QG_LINK_HELPERS")
    os.environ["QG_LINK_HELPERS"] = "1" if leaf.helpers else "0"
    try:
        if leaf.layer == "none":
            task = _abi.default_task()
            task.use_fall, task.fall_height, task.frame_skip = 1, 0.05, fs
            task.auto_reset, task.reset_flags = int(auto_reset), reset_flags
            sim, env = BatchedSim(n, model=model, task=task), None
        else:
            if leaf.layer == "po":
                env = POWalkingQuadrupedVecEnv(n, obs_window=obs_window, nan_direction=False, seed=seed, model_path=path, frame_skip=fs, **env_kw)
            else:
                env = WalkingQuadrupedVecEnv(n, nan_direction=False, seed=seed, model_path=path, frame_skip=fs, **env_kw)
            sim = env._sim
    finally:
        if old is None:
            del os.environ["QG_LINK_HELPERS"]
        else:
            os.environ["QG_LINK_HELPERS"] = old
    if leaf.mapping != "auto":
        sim.set_mapping(MAPPINGS[leaf.mapping])
    return sim, env


def _ragged_link(S):
    return link_max(S) - 3


def _one(S):
    return 1


def _first_quad(S):             # a four-wave-workgroup grid whose last workgroup holds ONE env
    return link_max(S) + 1


def _last_quad(S):
    return quad_max(S) - 1


def _first_pair(S):
    return quad_max(S) + 1


def _two_wave_quad(S):          # the one-leg-per-lane kernel at two waves per SIMD; the last workgroup holds ONE env
    return pair_max(S) + 1


def _explicit(S):               # explicit mapping requests on small grids: one-wave workgroups (and a ragged last wave)
    return 1000


def _name(family, *args):
    return "qg_step_kernel%s<%s>" % (family, ",".join(str(int(a)) for a in args))


LEAVES = {
    # the compiled-in robot, plain step
    _name("_link", 0, 0, 1, 0, 0): Leaf((_ragged_link, _one)),
    _name("_quad", 1, 1, 0, 4, 0, 0, 0): Leaf((_first_quad, _last_quad)),
    _name("_quad", 2, 1, 0, 4, 0, 0, 0): Leaf((_two_wave_quad,)),
    _name("_pair", 4, 0, 0): Leaf((_first_pair,)),
    _name("_quad", 1, 1, 0, 1, 0, 0, 0): Leaf((_explicit,), mapping="quad"),
    _name("_pair", 1, 0, 0): Leaf((_explicit,), mapping="pair"),
    _name("", 1): Leaf((_explicit,), mapping="lane"),
    # the compiled-in robot, walking
    _name("_link", 1, 0, 1, 1, 0): Leaf((_ragged_link,), layer="walk"),
    _name("_link", 1, 0, 1, 0, 0): Leaf((_ragged_link,), layer="walk", helpers=False),
    _name("_quad", 2, 1, 1, 4, 0, 1, 0): Leaf((_first_quad,), layer="walk"),
    _name("_quad", 1, 1, 1, 4, 0, 0, 0): Leaf((_first_quad,), layer="walk", helpers=False),
    _name("_quad", 1, 1, 1, 1, 0, 0, 0): Leaf((_explicit,), mapping="quad", layer="walk", helpers=False),
    _name("_quad", 2, 1, 1, 4, 0, 0, 0): Leaf((_two_wave_quad,), layer="walk"),
    _name("_pair", 4, 1, 0): Leaf((_first_pair,), layer="walk"),
    _name("_pair", 1, 1, 0): Leaf((_explicit,), mapping="pair", layer="walk"),
    # the compiled-in robot, partially observable
    _name("_link", 1, 1, 1, 1, 0): Leaf((_ragged_link,), layer="po"),
    _name("_link", 1, 1, 1, 0, 0): Leaf((_ragged_link,), layer="po", helpers=False),
    _name("_quad", 2, 1, 1, 4, 1, 1, 0): Leaf((_first_quad,), layer="po"),
    _name("_quad", 1, 1, 1, 4, 1, 0, 0): Leaf((_first_quad,), layer="po", helpers=False),
    _name("_quad", 2, 1, 1, 4, 1, 0, 0): Leaf((_two_wave_quad,), layer="po"),
    _name("_pair", 4, 1, 1): Leaf((_first_pair,), layer="po"),
    # any other robot: the table-driven kernels, with and without per-env dynamics rows
    _name("", 0): Leaf((_explicit,), robot="table", mapping="lane"),
}
for _dyn in (0, 1):
    LEAVES.update({
        _name("_link", 0, 0, 0, 0, _dyn): Leaf((_ragged_link,), robot="table", dyn=bool(_dyn)),
        _name("_link", 1, 0, 0, 0, _dyn): Leaf((_ragged_link,), robot="table", layer="walk", dyn=bool(_dyn)),
        _name("_link", 1, 1, 0, 0, _dyn): Leaf((_ragged_link,), robot="table", layer="po", dyn=bool(_dyn)),
        _name("_quad", 1, 0, 1, 4, 1, 0, _dyn): Leaf((_first_quad,), robot="table", layer="po", dyn=bool(_dyn)),
        _name("_quad", 1, 0, 1, 4, 0, 0, _dyn): Leaf((_first_quad,), robot="table", layer="walk", dyn=bool(_dyn)),
        _name("_quad", 1, 0, 0, 4, 0, 0, _dyn): Leaf((_first_quad,), robot="table", dyn=bool(_dyn)),
        _name("_quad", 1, 0, 1, 1, 0, 0, _dyn): Leaf((_explicit,), robot="table", mapping="quad", layer="walk", dyn=bool(_dyn)),
        _name("_quad", 1, 0, 0, 1, 0, 0, _dyn): Leaf((_explicit,), robot="table", mapping="quad", dyn=bool(_dyn)),
    })

# multi-step form -> (the tests/test_resident_gpu.py case that pins its rows bit for bit to per-launch steps, the per-launch leaf)
_SEQ = "tests.test_resident_gpu::test_sequence_launch_is_bit_identical_to_per_step_launches"
_OTHER = "tests.test_resident_gpu::test_sequence_and_resident_forms_with_other_model_numbers"
MULTI_TWINS = {
    _name("_link_multi", 1, 0): (_SEQ + "[4096-4-False]", _name("_link", 0, 0, 1, 0, 0)),
    _name("_link_multi", 1, 1): ("tests.test_resident_gpu::test_resident_closed_loop_is_bit_identical_to_per_step_launches[4096-1]",
                                 _name("_link", 0, 0, 1, 0, 0)),
    _name("_link_multi", 0, 0): (_OTHER, _name("_link", 0, 0, 0, 0, 0)),
    _name("_link_multi", 0, 1): (_OTHER, _name("_link", 0, 0, 0, 0, 0)),
    _name("_quad_multi", 1, 1): (_SEQ + "[8192-4-False]", _name("_quad", 1, 1, 0, 4, 0, 0, 0)),
    _name("_quad_multi", 2, 1): (_SEQ + "[40000-4-False]", _name("_quad", 2, 1, 0, 4, 0, 0, 0)),
    _name("_quad_multi", 1, 0): (_OTHER, _name("_quad", 1, 0, 0, 4, 0, 0, 0)),
    _name("_pair_multi", 4): (_SEQ + "[32768-4-False]", _name("_pair", 4, 0, 0)),
    _name("_pair_multi", 1): ("tests.test_resident_gpu::test_sequence_launch_in_the_explicit_pair_mapping", _name("_pair", 1, 0, 0)),
}
TWIN_PAIRS = {(multi, leaf) for multi, (_, leaf) in MULTI_TWINS.items()}


# ---- census of the launch sites ----------------------------------------------------------------------------------------------------
_KERNEL = {"lane": "qg_step_kernel", "link": "qg_step_kernel_link", "quad": "qg_step_kernel_quad", "pair": "qg_step_kernel_pair",
           "link_multi": "qg_step_kernel_link_multi", "quad_multi": "qg_step_kernel_quad_multi", "pair_multi": "qg_step_kernel_pair_multi"}


def _value(tok):
    tok = tok.strip()
    return {"true": 1, "false": 0}.get(tok, tok)


def launcher_parameters(src):
    """launcher family -> [(parameter name, default or None)] from the `template <..> static void launch_X(` declarations."""
    out = {}
    for params, fam in re.findall(r"template\s*<([^>]*)>\s*static\s+void\s+launch_(\w+)\s*\(", src):
        if fam not in _KERNEL:
            continue
        plist = []
        for p in params.split(","):
            decl, _, default = p.partition("=")
            plist.append((decl.split()[-1], _value(default) if default else None))
        out[fam] = plist
    return out


def _selector_bodies(src):
    """the bodies of the per-mapping selectors: `static void select_step_link(` .. and `void qg_select_step_pair(` .."""
    for m in re.finditer(r"void (?:qg_)?select_step_\w+\(", src):
        yield src[m.start():src.index("\n}\n", m.start())]


def launched_instantiations(src):
    """Every step-kernel name the launch sites can produce: the calls in the select_step_* functions and every launch_*_multi call,
    defaults filled in from the launcher declarations, DYN expanded to {0, 1}."""
    params = launcher_parameters(src)
    sites = [(m.group(1), m.group(2)) for body in _selector_bodies(src)
             for m in re.finditer(r"launch_(lane|link|quad|pair)<([^<>]*)>\s*\(", body)]
    sites += [(m.group(1), m.group(2)) for m in re.finditer(r"launch_((?:link|quad|pair)_multi)<([^<>]*)>\s*\(", src)]
    names = set()
    for fam, args in sites:
        given = [_value(a) for a in args.split(",")]
        plist = params[fam]
        assert len(given) <= len(plist), (fam, args)
        full = given + [d for _, d in plist[len(given):]]
        assert None not in full, (fam, args)
        choices = [(0, 1) if a == "DYN" else (int(a),) for a in full]
        for combo in product(*choices):
            names.add(_name(_KERNEL[fam][len("qg_step_kernel"):], *combo))
    return names
