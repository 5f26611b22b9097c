"""The device-side VecEnv wrappers stacked in every order a training run uses, through episode ends, on both paths
(tests/wrapper_stacks.py holds the stacks, the cases and the twin).

Every layer alone is held against float64 in its own module, so a stack is checked bit for bit against its twin: the same env class and
seed stepped bare, the layers' own handle calls made by hand on its rows in the stack's order.  Per step obs, reward, done,
terminal_obs, components and (under the command curriculum) ``commands_tensor`` are compared as uint32 words; after the last step every
layer's state -- the schedule's blob and the curriculum's blob, weights, counts and segments among them -- and a RewardMonitor fed the
stack's components against one fed the twin's.  The terminal rows under a normaliser wider than they are (stacks 2, 4, 8, 10, 11; at the
width ``O + 10`` where the gait schedule is inside the privileged wrapper) are also audited in float64: the formula of
tests/normalize_reference.py on the raw rows with the leading entries of the statistics the device reports, under the one-ulp output
rule of tests/test_normalize_gpu.py -- the only tolerance of the twin tests.

The twin runs the same kernels, so it checks plumbing.  The two layers that came last are tied, AS THE STACK DRIVES THEM, to their NumPy
definitions too: ``command_curriculum_reference.Curriculum`` replayed on the recorded done vectors and component columns gives the
weights, counts and segments exactly and the commands within ``command_tolerance(speed, MARGIN)``; the clock columns of the raw rows
follow ``gait_schedule_reference.Checker`` by the rule of tests/test_zz_gait_schedule_gpu.py (``check_columns``).

The NumPy cold path runs the same stacks from a fresh stack of the same seed.  Its rows are those of the device path bit for bit for the
partially observable env, whose finished rows hold the reset stack on both paths.  For the plain and the walking env a finished env's
device row is its TERMINAL observation and the NumPy row the reset row (zeros): the envs' documented difference.  The normaliser's
statistics see those rows, so from the first episode end on the two paths part in every normalised observation column; what does not
pass through those statistics (rewards, dones, the raw rows of the running envs, stack 5's privileged columns, the component columns the
curriculum judges) stays bit-equal and is asserted so, and the normalised rows are held against ``Twin(cold=True)``, which states the
cold path's row (wrapper_stacks.py).

The last test runs stack 5 around the plain env and stack 10 around both walking envs twice more: eagerly with ``stream=side`` passed
to ``step_tensor`` and ``monitor.record`` while torch's current stream stays the default one, and as a one-step captured graph replayed
24 times.  Both equal the default-stream run bit for bit in every output and every layer's final state.

Every case prints how many env-steps finished and asserts that envs finished on at least two distinct steps; the new cases print and
assert the counts that keep them from passing empty (segments ended by ``done`` and by ``resample_steps``, successes and failures,
weights that moved, the gate saying "stand" and "go", criteria of different kinds disagreeing).  The module's name keeps it with its
neighbours at the end of collection, as the other modules that capture hipGraphs on a side stream."""
import collections
import functools

import numpy as np
import pytest
import torch

import command_curriculum_reference as C
import gait_schedule_reference as GS
import wrapper_stacks as S

from quadruped_gym_amd.curriculum import DeviceCommandCurriculumVecEnv
from quadruped_gym_amd.gait import DeviceGaitRewardVecEnv
from quadruped_gym_amd.normalize import DeviceVecNormalize
from quadruped_gym_amd.perturb import DevicePerturbedVecEnv
from quadruped_gym_amd.privileged import DevicePrivilegedVecEnv
from quadruped_gym_amd.schedule import DeviceGaitScheduleVecEnv

pytestmark = pytest.mark.gpu
N, STEPS = S.N, S.STEPS
IDS = [f"stack{s}-{k}" for s, k in S.CASES]
WIDE_NORMALISER = [(s, k) for s, k in S.CASES if "priv" in S.STACKS[s][:-1]]       # the normaliser outside the privileged wrapper
CURRICULUM = [(s, k) for s, k in S.CASES if "cur" in S.STACKS[s]]
SCHEDULE = [(s, k) for s, k in S.CASES if "sched" in S.STACKS[s]]
STEP_KEYS = ("obs", "reward", "terminal_obs", "components", "packed", "commands")
PARTS = ("norm", "perturbation", "contact", "monitor", "schedule", "curriculum")
_ids = lambda cases: [f"stack{s}-{k}" for s, k in cases]


def _same_tree(a, b):
    """Two states (nested dicts of arrays, numbers and None) hold the same bytes."""
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same_tree(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _assert_finished(what, steps):
    finished, when = S.finished_steps(steps)
    print("%s: %d env-steps finished, on steps %s" % (what, finished, when))
    assert finished > 0 and len(when) >= 2, (finished, when)


# ---- the NumPy definitions of the two new layers, replayed on what the stack recorded --------------------------------------------------------
def _initial_weights():
    """The bins whose speed interval meets ``initial_speed`` start at ``weight_max``, the others at 0 (on the reference's own edges)."""
    edges, _ = C.edges(S.CUR["speed"], S.CUR["bins"])
    lo, hi = (np.float32(s) for s in S.CUR["initial_speed"])
    meets = (edges[:-1] <= hi) & (edges[1:] >= lo)
    return tuple(int(w) for w in np.repeat(np.where(meets, S.CUR["weight_max"], 0), S.CUR["bins"][1]))


def _reference_curriculum(run, rows):
    return C.Curriculum(N, S.CUR["speed"], S.CUR["bins"], _initial_weights(), S.CUR["weight_max"], S.CUR["delta"], S.CUR["resample_steps"],
                        S.CUR["min_steps"], tuple(rows), None, S.CUR["seed"], run["env_index_base"])


def _judged_columns(stack_id, kind):
    """The columns of the stack's component rows that the curriculum reads: those of the layers inside it, by key."""
    layers = S.STACKS[stack_id]
    keys = S.reward_keys(layers, kind)
    return [keys.index(key) for key in S.reward_keys(layers[:layers.index("cur")], kind)]


@functools.lru_cache(maxsize=None)
def _curriculum_replay(stack_id, kind):
    """``command_curriculum_reference.Curriculum`` on the recorded ``done`` and component columns of the stack's device path.  After
    the reset and after every step the integers equal the device's exactly and the four command floats lie within the measured
    budget.  Returns what each launch decided, and per criterion which segments passed it (a reference with that criterion alone:
    segments, steps and sums do not depend on the weights)."""
    run = S.device_run(stack_id, kind)
    rows = S.criteria_rows(S.STACKS[stack_id], kind)
    columns = _judged_columns(stack_id, kind)
    ref, single = _reference_curriculum(run, rows), [_reference_curriculum(run, [row]) for row in rows]
    for r in [ref] + single:
        r.begin()                                               # the stack's reset() began a new segment for every env

    def check(what, got, commands):
        for key, want in (("weights", ref.weight), ("episodes", ref.episodes), ("successes", ref.successes), ("bin", ref.bin),
                          ("steps", ref.steps), ("segment", ref.segment)):
            assert np.array_equal(got[key], want), (what, key)
        err, tol = np.abs(commands.astype(np.float64) - ref.commands()[:, :4]), C.command_tolerance(ref.speed, C.MARGIN)[:, :4]
        assert (err <= tol).all(), (what, (err / tol).max())
        return float((err / tol).max())

    worst = check("reset", run["reset_curriculum"], run["reset_commands"][0])
    outs, passed = [], []
    for t, got in enumerate(run["stack"]):
        comps = got["components"][:, columns]
        outs.append(ref.advance(got["done"], comps))
        passed.append(np.stack([r.advance(got["done"], comps)["success"] for r in single]))
        worst = max(worst, check("step %d" % t, run["curriculum"][t], got["commands"]))
    return {"outs": outs, "passed": passed, "worst": worst, "initial": np.array(_initial_weights()), "ref": ref}


def _assert_curriculum_conditions(stack_id, kind):
    replay = _curriculum_replay(stack_id, kind)
    outs, ref = replay["outs"], replay["ref"]
    by_done = sum(int((o["ended"] & o["by_done"]).sum()) for o in outs)
    by_length = sum(int((o["ended"] & ~o["by_done"]).sum()) for o in outs)
    moved = int((ref.weight != replay["initial"]).sum())
    print("stack %d around the %s env, curriculum: %d segments ended by done, %d by resample_steps; episodes %s, successes %s; %d weights "
          "moved; the commands' largest share of MARGIN x budget %.3f" % (stack_id, kind, by_done, by_length, ref.episodes.tolist(),
                                                                       ref.successes.tolist(), moved, replay["worst"]))
    assert by_done >= 1 and by_length >= 1
    assert (ref.successes < ref.episodes).any() and ref.successes.sum() > 0
    assert moved >= 1
    if stack_id == 10:                                          # three kinds of criteria: they do not all say the same
        passed = np.concatenate(replay["passed"], axis=1)       # [kind, every (step, env)]
        long_enough = np.concatenate([o["ended"] & (o["before_steps"] >= S.CUR["min_steps"]) for o in _with_steps(outs)])
        split = long_enough & passed.any(axis=0) & ~passed.all(axis=0)
        print("stack 10 around the %s env: segments passed per kind (base, gait, schedule) %s of %d judged; %d where one kind fails and "
              "another passes" % (kind, passed[:, long_enough].sum(axis=1).tolist(), int(long_enough.sum()), int(split.sum())))
        assert passed.shape[0] == 3 and split.any()
        counts = passed[:, long_enough].sum(axis=1)
        assert (counts > 0).all() and (counts < long_enough.sum()).all()        # and every kind passes somewhere and fails somewhere


def _with_steps(outs):
    """Each launch's decision with the length its segments had: the reference resets ``steps`` of an ended segment, so it is counted
    here from the decisions themselves."""
    steps, result = np.zeros(N, np.int64), []
    for o in outs:
        steps = steps + 1
        result.append(dict(o, before_steps=steps.copy()))
        steps = np.where(o["ended"], 0, steps)
    return result


def _assert_gate_conditions(stack_id, kind, run):
    stand = sum(int(s["stand"].sum()) for s in run["twin"])
    go = sum(int((~s["stand"]).sum()) for s in run["twin"])
    print("stack %d around the %s env: the schedule's gate said stand on %d env-steps, go on %d" % (stack_id, kind, stand, go))
    assert stand >= 1 and go >= 1


# ---- 1. the device path against the twin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stack_id,kind", S.CASES, ids=IDS)
def test_device_path_is_the_twin_bit_for_bit(stack_id, kind):
    run = S.device_run(stack_id, kind)
    layers = S.STACKS[stack_id]
    first, want_first = run["reset"]
    assert first.shape == (N, run["obs_dim"]) and S.same(first, want_first)
    if "cur" in layers:
        assert S.same(*run["reset_commands"])
    for t, (got, want) in enumerate(zip(run["stack"], run["twin"])):
        assert np.array_equal(got["done"], want["done"]), t
        for key in STEP_KEYS:
            assert (key in got) == (key in want), (t, key)
            if key in got:
                assert S.same(got[key], want[key]), (t, key)
        assert got["obs"].shape == (N, run["obs_dim"])
        if "terminal_obs" in got:
            assert got["terminal_obs"].shape == (N, run["terminal_dim"])
    assert ("terminal_obs" in run["stack"][0]) == (kind == "po") and ("components" in run["stack"][0]) == (kind != "plain")
    assert ("commands" in run["stack"][0]) == ("cur" in layers)
    _assert_finished("stack %d around the %s env, device path" % (stack_id, kind), run["stack"])
    got, want = run["final"]
    for part in PARTS:
        assert _same_tree(got[part], want[part]), part
    assert (got["perturbation"] is not None) == ("perturb" in layers) and (got["contact"] is not None) == ("gait" in layers or "sched" in layers)
    assert (got["schedule"] is not None) == ("sched" in layers) and (got["curriculum"] is not None) == ("cur" in layers)
    assert (got["monitor"] is not None) == (kind != "plain")
    if got["monitor"] is not None:
        assert got["monitor"]["records"] == STEPS and got["monitor"]["episodes"] == S.finished_steps(run["stack"])[0]
    if "cur" in layers:
        _assert_curriculum_conditions(stack_id, kind)
    if "sched" in layers and kind == "po":
        _assert_gate_conditions(stack_id, kind, run)


# ---- 2. the terminal rows under the wide normaliser, in float64 -----------------------------------------------------------------------------
@pytest.mark.parametrize("stack_id,kind", WIDE_NORMALISER, ids=_ids(WIDE_NORMALISER))
def test_terminal_rows_against_the_float64_formula(stack_id, kind):
    """A finished env's terminal row has the actor's columns -- the env's O, and the ten clock columns where the gait schedule is
    inside the privileged wrapper: the buffer ``terminal_obs`` of the partially observable env, the leading columns of the row itself
    for the walking env.  Raw as the twin saw them, the statistics as the device reports them after that step, the leading entries of
    mean and var."""
    run = S.device_run(stack_id, kind)
    A = run["O"] + (10 if "sched" in S.STACKS[stack_id] else 0)
    assert run["obs_dim"] == A + 85 and run["terminal_dim"] == A < run["obs_dim"]
    rows = clipped = 0
    worst = 0.0
    for t, (got, want) in enumerate(zip(run["stack"], run["twin"])):
        fin = got["done"]
        if not fin.any():
            continue
        sd = run["stats"][t]
        assert sd["obs_rms.mean"].shape == (A + 85,)
        if kind == "po":
            out, raw = got["terminal_obs"][fin], want["raw"]["terminal_obs"][fin]
        else:
            out, raw = got["obs"][fin, :A], want["raw"]["obs"][fin, :A]
        assert raw.shape == (int(fin.sum()), A) and np.isfinite(raw).all() and raw.any()
        err, over = S.audit_terminal_rows(out, raw, sd["obs_rms.mean"], sd["obs_rms.var"])
        rows, clipped, worst = rows + len(raw), clipped + over, max(worst, err)
    print("stack %d around the %s env: %d terminal rows %d wide, largest error %.3f ulp, %d clipped elements" % (stack_id, kind, rows, A, worst, clipped))
    assert rows > 0


# ---- 3. the NumPy cold path -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stack_id,kind", S.CASES, ids=IDS)
def test_numpy_path_through_the_same_steps(stack_id, kind):
    run = S.device_run(stack_id, kind)
    want_first, cold = S.cold_run(stack_id, kind)
    O, W, po = run["O"], run["obs_dim"], kind == "po"
    acts = S.actions().cpu().numpy()
    layers = S.STACKS[stack_id]
    stack = S.build_stack(layers, kind)
    norm = S.layer_of(stack, DeviceVecNormalize)
    cur = S.layer_of(stack, DeviceCommandCurriculumVecEnv)
    judged = _judged_columns(stack_id, kind) if cur is not None else None
    first = stack.reset()
    assert first.shape == (N, W) == (N, stack.obs_dim) and S.same(first, want_first) and S.same(first, run["reset"][0])
    parted = False                      # the two paths' statistics have seen different rows
    steps = []
    for t in range(STEPS):
        obs, rew, done, infos = stack.step(acts[t])
        dev, twin_dev, want = run["stack"][t], run["twin"][t], cold[t]
        done = np.asarray(done).astype(bool)
        steps.append({"done": done})
        live = ~done
        assert obs.shape == (N, W) and rew.shape == (N,) and done.shape == (N,)
        # what the statistics of the observations do not touch is the device path's, on every env
        assert np.array_equal(done, dev["done"]) and S.same(rew, dev["reward"]), t
        if stack_id == 5:
            assert S.same(obs[:, O:], dev["obs"][:, O:]), t                          # the privileged columns stay raw
        if cur is not None:             # the columns the curriculum judged are the device path's of the same keys, and so are its commands
            host = cur._host_components()
            assert host.shape == (N, len(judged)) and host.dtype == np.float32 and S.same(host, dev["components"][:, judged]), t
            assert S.same(cur.commands_tensor.cpu().numpy(), dev["commands"]), t
        # the rows: the cold path's statement on every env, a finished env's reset row included
        assert S.same(obs, want["obs"]), t
        parted = parted or (not po and bool(done.any()))
        if not parted:
            assert S.same(obs[live], dev["obs"][live]), t
        # the un-normalised rows of the outer normaliser
        raw_obs, raw_rew = norm.get_original_obs(), norm.get_original_reward()
        assert S.same(raw_obs, want["raw"]["obs"]) and S.same(raw_rew, want["raw"]["reward"]) and S.same(raw_rew, twin_dev["raw"]["reward"]), t
        assert S.same(raw_obs[live], twin_dev["raw"]["obs"][live]), t
        if done.any():
            if po:                      # both paths hold the reset stack
                assert S.same(raw_obs[done], twin_dev["raw"]["obs"][done]), t
            else:                       # the documented difference: the reset row is zeros, the device row the terminal observation
                assert not raw_obs[done][:, :O].any() and twin_dev["raw"]["obs"][done][:, :O].any(axis=1).all(), t
        for i in np.nonzero(done)[0]:
            term = infos[int(i)].get("terminal_observation")
            assert term is not None, (t, i)
            term = np.asarray(term)
            assert term.shape == (run["terminal_dim"],) and term.dtype == np.float32 and np.isfinite(term).all(), (t, i, term.shape)
            assert S.same(term, want["terminal_obs"][i]), (t, i)
            if po:
                assert S.same(term, dev["terminal_obs"][i]), (t, i)
    _assert_finished("stack %d around the %s env, NumPy path" % (stack_id, kind), steps)
    if cur is not None:
        assert _same_tree(S.curriculum_state(cur.curriculum), run["final"][0]["curriculum"])
    stack.close()


# ---- 4. snapshot / restore / close over the full training stack -------------------------------------------------------------------------------
class _CountingLib:
    """The library as a handle sees it, counting the calls of the handle's own destroy function."""

    def __init__(self, lib, destroy, counts, key):
        self._lib, self._destroy, self._counts, self._key = lib, destroy, counts, key

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != self._destroy:
            return fn

        def counted(*args):
            self._counts[self._key] += 1
            return fn(*args)
        return counted


def _step_matches(got, want):
    fin = want["done"]
    return (np.array_equal(got["done"], fin) and all(S.same(got[k], want[k]) for k in ("obs", "reward", "components", "commands") if k in want)
            and ("commands" in got) == ("commands" in want)
            and ("terminal_obs" not in want or S.same(got["terminal_obs"][fin], want["terminal_obs"][fin])))     # the finished envs' rows


SNAPSHOT_KEYS = {"perturb": "perturbation", "gait": "gait_reward", "sched": "gait_schedule", "cur": "command_curriculum", "priv": "privileged",
                 "norm": "normalizer"}


def _commands_in_force(stack):
    """``commands_tensor`` of the stack's curriculum is what the walking layer holds (or there is no curriculum)."""
    cur = S.layer_of(stack, DeviceCommandCurriculumVecEnv)
    return cur is None or S.same(cur.commands_tensor.cpu().numpy(), np.concatenate(cur.commands(), axis=1))


@pytest.mark.parametrize("stack_id,kind", [(4, "walk"), (4, "po"), (10, "walk"), (10, "po")], ids=["walk", "po", "stack10-walk", "stack10-po"])
def test_snapshot_restore_and_close_over_the_full_stack(stack_id, kind):
    layers = S.STACKS[stack_id]
    acts = S.actions()
    stack = S.build_stack(layers, kind)
    driver = S.StackDriver(stack, layers, kind)
    stack.reset()
    for t in range(9):
        driver.step(acts[t])
    snap = stack.snapshot()
    # a nesting of every wrapper's key around the env's own snapshot
    level = snap
    nesting = [SNAPSHOT_KEYS[name] for name in reversed(layers)]
    if stack_id == 10:
        assert nesting == ["normalizer", "privileged", "command_curriculum", "gait_schedule", "gait_reward", "perturbation"]
    for key in nesting:
        assert set(level) == {"env", key} | ({"training"} if key == "normalizer" else set()), (key, set(level))
        if key in ("privileged", "gait_reward"):
            assert level[key] == {}
        elif key in ("gait_schedule", "command_curriculum"):
            assert level[key].dtype == np.uint8 and level[key].size > 0
        level = level["env"]
    assert {"sim", "contact", "walk", "velocity", "heading"} <= set(level) and ("po" in level) == (kind == "po")
    assert snap["training"] is True
    first = [driver.step(acts[t]) for t in range(9, STEPS)]
    end = S.stack_final_state(stack, None)
    _assert_finished("stack %d around the %s env, steps 10 .. 24" % (stack_id, kind), first)
    # into a freshly built stack: steps 10 .. 24 repeat bit for bit
    fresh = S.build_stack(layers, kind)
    again = S.StackDriver(fresh, layers, kind)
    fresh.reset()
    fresh.restore(snap)
    assert _commands_in_force(fresh)
    for t in range(9, STEPS):
        assert _step_matches(again.step(acts[t]), first[t - 9]), t
    assert _same_tree(S.stack_final_state(fresh, None), end)
    # ... and so do they on the stack the snapshot was taken from
    stack.restore(snap)
    assert _commands_in_force(stack)
    for t in range(9, STEPS):
        assert _step_matches(driver.step(acts[t]), first[t - 9]), t
    assert _same_tree(S.stack_final_state(stack, None), end)
    driver.monitor.close(), again.monitor.close()
    fresh.close()
    # close: every layer handle is destroyed exactly once
    env = S.bottom(stack)
    gait = S.layer_of(stack, DeviceGaitRewardVecEnv).gait
    handles = {"normalizer": stack.normalizer, "privileged": S.layer_of(stack, DevicePrivilegedVecEnv).privileged, "gait": gait,
               "sensor": gait.sensor, "perturbation": S.layer_of(stack, DevicePerturbedVecEnv).perturbation, "sim": env._sim, "walk": env._walk}
    if kind == "po":
        handles["po"] = env._obs_pack
    if stack_id == 10:
        handles["schedule"] = S.layer_of(stack, DeviceGaitScheduleVecEnv).schedule
        handles["curriculum"] = S.layer_of(stack, DeviceCommandCurriculumVecEnv).curriculum
        assert handles["schedule"].sensor is handles["sensor"] and handles["curriculum"].walk is env._walk
    assert handles["sensor"] is env.contact_sensor(S.FORCE_THRESHOLD) and handles["privileged"] is env.privileged_state(S.FORCE_THRESHOLD)
    counts = collections.Counter()
    for key, h in handles.items():
        assert h._h is not None and h._destroy, key
        h._lib = _CountingLib(h._lib, h._destroy, counts, key)
    stack.close()
    assert all(h._h is None for h in handles.values()) and env._sim is None
    assert counts == {key: 1 for key in handles}, counts
    stack.close()                                                   # a second close is harmless
    assert counts == {key: 1 for key in handles}, counts


# ---- 5. the two new layers against their NumPy definitions, as the stack drives them -----------------------------------------------------------
@pytest.mark.parametrize("stack_id,kind", CURRICULUM, ids=_ids(CURRICULUM))
def test_curriculum_in_the_stack_is_the_numpy_definition(stack_id, kind):
    """The reference replayed on the recorded done vectors and component columns: weights, episodes, successes, bin, steps and
    segment exactly after every step, the commands within ``command_tolerance(speed, MARGIN)`` (the asserts live in the replay)."""
    replay = _curriculum_replay(stack_id, kind)
    judged = sum(int(o["ended"].sum()) for o in replay["outs"])
    print("stack %d around the %s env: %d segments judged, %d succeeded; the commands' largest share of MARGIN x budget %.3f"
          % (stack_id, kind, judged, int(replay["ref"].successes.sum()), replay["worst"]))
    assert judged == replay["ref"].episodes.sum() > N and len(replay["outs"]) == STEPS


@pytest.mark.parametrize("stack_id,kind", SCHEDULE, ids=_ids(SCHEDULE))
def test_clock_columns_in_the_stack_follow_the_numpy_oscillator(stack_id, kind):
    """The ten clock columns of the raw rows, as the twin saw them in front of the normaliser, against the exact-integer oscillator:
    the reset rows, every step's rows and, for the partially observable env, the finished envs' terminal rows (the old episode's)."""
    run = S.device_run(stack_id, kind)
    O = run["O"]
    chk = GS.Checker(N, done_row="reset" if kind == "po" else "terminal", seed=S.SCHED_SEED, env_index_base=run["env_index_base"],
                     dt32=run["dt32"], **GS.PARAMS)
    view, _ = chk.begin()
    worst = GS.check_columns("reset", run["raw_reset"][:, O:O + 10], view)
    terminal = 0
    for t, want in enumerate(run["twin"]):
        fin = want["done"]
        row, old = chk.step(fin)
        worst = max(worst, GS.check_columns("step %d rows" % t, want["raw"]["obs"][:, O:O + 10], row))
        if kind == "po" and fin.any():
            worst = max(worst, GS.check_columns("step %d terminal rows" % t, want["raw"]["terminal_obs"][fin, O:O + 10],
                                                {k: v[fin] for k, v in old.items()}))
            terminal += int(fin.sum())
    print("stack %d around the %s env: clock columns' largest |gpu - f64| %.3e (bound %.1e); %d terminal rows; episodes up to %d"
          % (stack_id, kind, worst, GS.MARGIN * GS.BUDGET_CLOCK, terminal, int(chk.episode.max())))
    assert chk.episode.min() >= 2 and (kind != "po" or terminal > 0)


# ---- 6. a side stream and a captured graph -------------------------------------------------------------------------------------------------------
STREAM_CASES = [(5, "plain"), (10, "walk"), (10, "po")]


@pytest.fixture(scope="module")
def side():
    """One side stream for the module, taken once."""
    return torch.cuda.Stream(S.DEV)


def _assert_run_equals(what, steps, final, run):
    for t, (got, want) in enumerate(zip(steps, run["stack"])):
        assert np.array_equal(got["done"], want["done"]), (what, t)
        for key in STEP_KEYS:
            assert (key in got) == (key in want), (what, t, key)
            if key in got:
                assert S.same(got[key], want[key]), (what, t, key)
    assert len(steps) == STEPS
    for part in PARTS:
        assert _same_tree(final[part], run["final"][0][part]), (what, part)


@pytest.mark.parametrize("stack_id,kind", STREAM_CASES, ids=_ids(STREAM_CASES))
def test_side_stream_and_graph_replay_are_the_default_stream_run(stack_id, kind, side):
    """The same 24 steps three times: ``device_run`` on the default stream; eagerly with ``stream=side`` passed to ``step_tensor``
    and ``monitor.record`` while torch's current stream stays the default one; a one-step captured graph replayed 24 times.  In the
    eager run the side stream is held back by a matrix product ahead of every step, so a launch or copy a wrapper left on another
    stream runs ahead of the env's launch instead of behind it."""
    run = S.device_run(stack_id, kind)
    layers = S.STACKS[stack_id]
    acts = S.actions()
    big, product = torch.ones((2048, 2048), device=S.DEV), torch.empty((2048, 2048), device=S.DEV)

    # eagerly on the side stream
    stack = S.build_stack(layers, kind)
    driver = S.StackDriver(stack, layers, kind, static=True)
    assert S.same(stack.reset(), run["reset"][0])
    torch.cuda.synchronize()
    steps = []
    for t in range(STEPS):
        with torch.cuda.stream(side):
            torch.mm(big, big, out=product)
        steps.append(driver.step(acts[t], stream=side))
    monitor = getattr(driver, "monitor", None)
    _assert_run_equals("side stream", steps, S.stack_final_state(stack, monitor), run)
    if monitor is not None:
        monitor.close()
    stack.close()

    # a one-step graph: a warm-up step, so every lazily allocated buffer exists; the capture; then back to the fresh state
    stack = S.build_stack(layers, kind)
    driver = S.StackDriver(stack, layers, kind, static=True)
    monitor = getattr(driver, "monitor", None)
    assert S.same(stack.reset(), run["reset"][0])
    snap, fresh_monitor = stack.snapshot(), monitor.state() if monitor is not None else None
    s_act = torch.zeros((N, 12), device=S.DEV)
    s_act.copy_(acts[0])
    driver.step(s_act, stream=side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        driver.launch(s_act, stream=side)
    stack.restore(snap)                                         # whatever a capture may have run, start from the fresh state
    if monitor is not None:
        monitor.load_state(fresh_monitor)
    for buf in driver.buffers():
        buf.zero_()
    assert _commands_in_force(stack)
    steps = []
    for t in range(STEPS):
        s_act.copy_(acts[t])
        torch.cuda.synchronize()
        graph.replay()
        steps.append(driver.read())
    _assert_run_equals("graph replay", steps, S.stack_final_state(stack, monitor), run)
    del graph
    if monitor is not None:
        monitor.close()
    stack.close()
