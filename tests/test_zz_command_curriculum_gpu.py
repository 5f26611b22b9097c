"""The command curriculum on the GPU (qg_cmdcur_*, csrc/qg_cmdcur.hip) against tests/command_curriculum_reference.py.  Over the scripted
table of done and components rows -- inputs of the launch, so no physics scripts them -- bin, steps, segment, weights, episodes and
successes equal the reference EXACTLY after every launch; speed, alpha and theta are pure functions of (key, bin, segment), so the
reference's float32 values are the device's, and the six command floats -- four through qg_walk_get_commands and command_out, which
agree bit for bit, the global velocity through the walking layer's snapshot -- stay within MARGIN x the CPU-measured float32 budget of
their float64 evaluation.  Then the next env-step's reward terms and partially observable frames, begin, strides and done kinds, graph
replay, the state blob, set_weights, the refusals and the wrapper in stacks.
The module's name puts it last in collection, as the other modules that capture hipGraphs on a side stream."""
import ctypes as C

import numpy as np
import pytest
import torch

import command_curriculum_reference as R

from quadruped_gym_amd import _abi
from quadruped_gym_amd.curriculum import CommandCurriculum, DeviceCommandCurriculumVecEnv
from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv, WalkingQuadrupedVecEnv
from quadruped_gym_amd.gait import DeviceGaitRewardVecEnv
from quadruped_gym_amd.normalize import DeviceVecNormalize

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WALK_BLOB_HEADER = 24                                      # the walking layer's snapshot: header, then vel, head, gvel, each [2][n] f32
CASES = {"main": R.MAIN, "one": R.ONE, "wide": R.WIDE}


def _dev(a, dtype=None):
    return torch.from_numpy(np.array(a, dtype=dtype)).to(DEV)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _env(n, **kw):
    env = WalkingQuadrupedVecEnv(n, **dict(dict(nan_direction=False, max_time=0.05), **kw))
    env.reset()
    return env


def _cur(env, params, **kw):
    return CommandCurriculum(env._walk, **dict(params, **kw))


def _six(env):
    """[n, 6] float32 (vx, vy, hx, hy, gvx, gvy): four through qg_walk_get_commands, the global velocity from the layer's snapshot."""
    n = env.num_envs
    velocity, heading = (a.copy() for a in env.commands())
    blob = env._walk.state()
    gvel = blob[WALK_BLOB_HEADER + 16 * n:WALK_BLOB_HEADER + 24 * n].view(np.float32).reshape(2, n).T
    return np.concatenate([velocity, heading, gvel], axis=1)


def _check_state(what, cur, ref):
    got, stats = cur.bins(), cur.stats()
    assert np.array_equal(got["bin"], ref.bin) and np.array_equal(got["steps"], ref.steps) and np.array_equal(got["segment"], ref.segment), what
    assert np.array_equal(cur.weights().ravel(), ref.weight), what
    assert np.array_equal(stats["episodes"].ravel(), ref.episodes) and np.array_equal(stats["successes"].ravel(), ref.successes), what


def _check_commands(what, env, ref, command_out=None):
    """The six floats within MARGIN x the budget of float64 on the reference's float32 (speed, alpha, theta); command_out's bits are
    qg_walk_get_commands'.  Returns the largest share of the bound."""
    six = _six(env)
    if command_out is not None:
        assert _same(command_out, six[:, :4]), what
    err, tol = np.abs(six.astype(np.float64) - ref.commands()), R.command_tolerance(ref.speed, R.MARGIN)
    assert (err <= tol).all(), (what, (err / tol).max())
    return six, float((err / tol).max())


# ---- 1. the scripted table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["main", "one", "wide"])
def test_scripted_table_is_the_reference(case):
    """main: uint8 done, contiguous rows.  wide: float32 done at a stride, components and command_out as column slices of wider rows,
    theta drawn.  one: bool done, no criteria and no components."""
    params, n = CASES[case], R.SIZES[case]
    env = _env(n)
    cur, ref = _cur(env, params), R.Curriculum(n, **params)
    _check_state("new handle", cur, ref)                      # segment 0 drawn at create, its command written
    six, worst = _check_commands("new handle", env, ref)
    for got, want in zip(cur.grid(), R.edges(params["speed"], params["bins"])):
        assert _same(got, want)
    done, comps = R.table(n)
    strided = case == "wide"
    d_done = torch.zeros((n, 3), device=DEV) if strided else torch.zeros(n, dtype=torch.bool if case == "one" else torch.uint8, device=DEV)
    d_comps = torch.full((n, R.N_COLUMNS + 2), 7.0, device=DEV) if strided else torch.zeros((n, R.N_COLUMNS), device=DEV)
    d_out = torch.full((n, 6), -3.0, device=DEV) if strided else torch.zeros((n, 4), device=DEV)
    v_done, v_comps, v_out = (d_done[:, 1], d_comps[:, 1:1 + R.N_COLUMNS], d_out[:, 1:5]) if strided else (d_done, d_comps, d_out)
    ended_total = 0
    for t in range(R.STEPS):
        v_done.copy_(_dev(done[t]).to(v_done.dtype))
        v_comps.copy_(_dev(comps[t]))
        cur.step(v_done, None if case == "one" else v_comps, v_out)
        out = ref.advance(done[t], comps[t])
        what = "%s step %d" % (case, t + 1)
        _check_state(what, cur, ref)
        before = six
        six, share = _check_commands(what, env, ref, v_out.cpu().numpy())
        worst = max(worst, share)
        keep = ~out["ended"]
        assert _same(six[keep], before[keep]), what           # an env whose segment did not end keeps its command bits
        ended_total += int(out["ended"].sum())
    if strided:                                               # nothing written outside the slices
        assert (d_out[:, 0] == -3.0).all() and (d_out[:, 5] == -3.0).all() and (d_comps[:, 0] == 7.0).all() and (d_comps[:, -1] == 7.0).all()
    assert ended_total == ref.episodes.sum() > (n if params["resample_steps"] else 0)      # (without resampling: the done rows alone)
    print("%s: %d envs, %d segments judged; the command floats' largest share of MARGIN x budget %.3f" % (case, n, ended_total, worst))
    env.close()
    assert cur._h is None


# ---- 2. the env-step that follows ------------------------------------------------------------------------------------------------------------
def test_next_walking_step_rewards_the_new_command():
    """Two walking envs step the same actions; one's commands are the curriculum's, the twin's are set from them through
    qg_walk_set_commands after every advance.  The reward terms that read the command (direction, speed, heading) and the observations
    agree bit for bit, so the step reads the slots the curriculum wrote -- and the commands do change, inside episodes too."""
    n = 70
    env, twin = _env(n), _env(n)
    cur = _cur(env, R.MAIN, resample_steps=3, criteria=(), min_steps=1)
    twin.set_commands(*env.commands())
    bufs = [[torch.zeros((n, 33), device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV),
             torch.zeros((n, 11), device=DEV)] for _ in range(2)]
    out = torch.zeros((n, 4), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    changed = finished = 0
    last = np.concatenate(env.commands(), axis=1).copy()
    for t in range(8):
        a = torch.rand((n, 12), generator=gen, device=DEV) * 2 - 1
        env.step_tensor(a, *bufs[0])
        twin.step_tensor(a, *bufs[1])
        cur.step(bufs[0][2], None, out)
        torch.cuda.synchronize()
        assert torch.equal(bufs[0][0], bufs[1][0]) and torch.equal(bufs[0][2], bufs[1][2]), t
        assert _same(bufs[0][3][:, 2:5].cpu().numpy(), bufs[1][3][:, 2:5].cpu().numpy()), t
        now = np.concatenate(env.commands(), axis=1).copy()
        assert _same(out.cpu().numpy(), now)
        changed += int((now != last).any(axis=1).sum())
        finished += int(bufs[0][2].sum())
        last = now
        twin.set_commands(now[:, :2], now[:, 2:])
    assert finished >= n and changed > finished               # episode ends, and resampling inside episodes on top
    assert changed <= cur.stats()["episodes"].sum()           # a command changes only where a segment was judged
    env.close(), twin.close()


def test_po_frames_show_the_command_in_force_and_reset_rows_the_old_one():
    """After env-step t the newest frame's command columns -- of a live env's row and of a finished env's reset row alike -- hold the
    command that was in force during the step, that is command_out of advance t - 1; the new one shows from step t + 1 on."""
    n, window = 70, 2
    env = POWalkingQuadrupedVecEnv(n, obs_window=window, nan_direction=False, max_time=0.05)
    env.reset()
    cur = _cur(env, R.MAIN, criteria=(), min_steps=1, resample_steps=4)
    D, lo = env.obs_dim, (window - 1) * env.FRAME + 23
    obs, term = torch.zeros((n, D), device=DEV), torch.zeros((n, D), device=DEV)
    rew, done = torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
    out = torch.zeros((n, 4), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(6)
    in_force = np.concatenate(env.commands(), axis=1).copy()
    finished = changed = 0
    for t in range(9):
        a = torch.rand((n, 12), generator=gen, device=DEV) * 2 - 1
        env.step_tensor(a, obs, rew, done, terminal_obs=term)
        cur.step(done, None, out)
        torch.cuda.synchronize()
        rows, fin = obs.cpu().numpy(), done.cpu().numpy() != 0
        assert _same(rows[:, lo:lo + 2], in_force[:, :2]), t                       # live rows and reset rows: the command of the step
        assert _same(term.cpu().numpy()[fin][:, lo:lo + 2], in_force[fin, :2]), t
        new = out.cpu().numpy().copy()
        changed += int((new != in_force).any(axis=1).sum())
        finished += int(fin.sum())
        in_force = new
    assert finished >= n and changed > finished
    env.close()


# ---- 3. begin, set_weights, the state blob ---------------------------------------------------------------------------------------------------
def test_begin_with_a_mask_and_set_weights():
    n = 300
    env = _env(n)
    cur, ref = _cur(env, R.MAIN), R.Curriculum(n, **R.MAIN)
    done, comps = R.table(n)
    for t in range(7):                                        # into the second segments, some bins unlocked
        cur.step(_dev(done[t]), _dev(comps[t]))
        ref.advance(done[t], comps[t])
    before = _six(env)
    mask = np.arange(n) % 3 == 1
    cur.begin(_dev(mask, np.uint8))
    ref.begin(mask)
    _check_state("masked begin", cur, ref)                    # segment + 1, steps 0, no count, no weight moved
    six, _ = _check_commands("masked begin", env, ref)
    assert _same(six[~mask], before[~mask])
    cur.begin()
    ref.begin()
    _check_state("begin of all", cur, ref)
    # the sums were dropped with the segments: the next launches judge as the reference does
    w = np.zeros(12, np.int32)
    w[[5, 10]] = (1, 12)
    cur.set_weights(w.reshape(3, 4))
    ref.weight = w.astype(np.int64)
    assert np.array_equal(cur.weights().ravel(), w)
    cur.begin()
    ref.begin()
    _check_state("after set_weights", cur, ref)
    assert set(np.unique(cur.bins()["bin"])) == {5, 10}       # every draw from the two bins that hold a weight
    for t in range(7, 14):
        cur.step(_dev(done[t]), _dev(comps[t]))
        ref.advance(done[t], comps[t])
        _check_state("step %d after set_weights" % (t + 1), cur, ref)
    for bad in (np.zeros(12, np.int32), np.full(12, 13, np.int32), np.ones(11, np.int32)):
        with pytest.raises(ValueError):
            cur.set_weights(bad)
    lib = _abi.load_library()                                 # the ABI's own validation, past the Python check
    assert lib.qg_cmdcur_set_weights(cur._h, np.zeros(12, np.int32).ctypes.data) == -1 and b"no bin with a weight" in lib.qg_last_error()
    assert lib.qg_cmdcur_set_weights(cur._h, np.full(12, -1, np.int32).ctypes.data) == -1
    _check_state("refused set_weights", cur, ref)
    env.close()


def test_state_blob_round_trip_continues_bit_for_bit():
    n = 300
    env = _env(n)
    cur = _cur(env, R.MAIN)
    done, comps = R.table(n)
    out = torch.zeros((n, 4), device=DEV)

    def run(lo, hi):
        rows = []
        for t in range(lo, hi):
            cur.step(_dev(done[t]), _dev(comps[t]), out)
            rows.append((out.cpu().numpy().tobytes(), cur.state().tobytes(), env._walk.state().tobytes()))
        return rows

    run(0, 9)
    blob, walk = cur.state(), env._walk.state()
    assert blob.size == cur.state_bytes() and np.array_equal(blob, cur.state())
    first = run(9, 20)
    assert first[-1][1] != blob.tobytes()
    cur.load_state(blob)
    env._walk.load_state(walk)
    assert np.array_equal(cur.state(), blob)                  # the round trip is exact
    assert run(9, 20) == first
    with pytest.raises(ValueError):
        cur.load_state(np.zeros(10, np.uint8))
    other = _env(70)
    small = _cur(other, R.MAIN)
    assert _abi.load_library().qg_cmdcur_set_state(small._h, blob.ctypes.data) == -1      # another shape's blob
    other.close(), env.close()


# ---- 4. graph replay ---------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_launches():
    n, K = 300, 14
    envs = [_env(n), _env(n)]
    curs = [_cur(e, R.MAIN) for e in envs]
    done, comps = R.table(n)
    d_done, d_comps = torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros((n, R.N_COLUMNS), device=DEV)
    outs = [torch.zeros((n, 4), device=DEV) for _ in range(2)]
    for c, o in zip(curs, outs):                              # one eager launch on both, so the capture is not the first use
        c.step(_dev(done[0]), _dev(comps[0]), o)
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=side):
        curs[1].step(d_done, d_comps, outs[1])
    assert np.array_equal(curs[0].state(), curs[1].state())   # a capture runs nothing
    for t in range(1, K + 1):
        curs[0].step(_dev(done[t]), _dev(comps[t]), outs[0])
        d_done.copy_(_dev(done[t])), d_comps.copy_(_dev(comps[t]))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]), t
    assert np.array_equal(curs[0].state(), curs[1].state()) and np.array_equal(envs[0]._walk.state(), envs[1]._walk.state())
    assert curs[1].stats()["episodes"].sum() > n              # the replays advanced the curriculum
    del graph
    for e in envs:
        e.close()


# ---- 5. the refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    n = 70
    env = _env(n)
    lib = _abi.load_library()
    cur = _cur(env, R.MAIN)
    s0, w0 = cur.state(), env._walk.state()
    comps, done, out = torch.zeros((n, 7), device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros((n, 4), device=DEV)
    adv = lambda *a: lib.qg_cmdcur_advance_device(cur._h, *a, None)
    for args, word in (((done.data_ptr(), 0, 1, comps.data_ptr(), 7, 5, None, 4), b"is not one of the 5 columns"),
                       ((done.data_ptr(), 0, 1, None, 7, 7, None, 4), b"without components"),
                       ((done.data_ptr(), 0, 1, comps.data_ptr(), 6, 7, None, 4), b"components_stride"),
                       ((done.data_ptr(), 0, 1, comps.data_ptr(), 7, -1, None, 4), b"n_columns"),
                       ((done.data_ptr(), 2, 1, comps.data_ptr(), 7, 7, None, 4), b"done_kind"),
                       ((done.data_ptr(), 0, 0, comps.data_ptr(), 7, 7, None, 4), b"done_stride"),
                       ((done.data_ptr(), 0, 1, comps.data_ptr(), 7, 7, out.data_ptr(), 3), b"command_out_stride")):
        assert adv(*args) == -1 and word in lib.qg_last_error(), word
    with pytest.raises(ValueError, match="a criterion reads column 5"):
        cur.step(done, comps[:, :5])
    for bad in (dict(components=torch.zeros((n - 1, 7), device=DEV)), dict(components=comps.double()), dict(components=comps.t()[:, :n].t()[:, ::2]),
                dict(command_out=torch.zeros((n, 3), device=DEV)), dict(done=torch.zeros(n, dtype=torch.int32, device=DEV))):
        kw = dict(dict(done=done, components=comps), **bad)
        with pytest.raises(ValueError):
            cur.step(kw["done"], kw["components"], kw.get("command_out"))
    # while the curriculum is bound: no in-kernel sampler, no second curriculum, no destroy of the layer under it
    sampler = _abi.QgCommandSampler.from_options({"min_speed": 0.0, "max_speed": 0.5})
    with pytest.raises(_abi.QuadGymError, match="a command curriculum is bound"):
        env._walk.set_command_sampler(sampler)
    assert lib.qg_walk_set_command_sampler(env._walk._h, None) == 0                        # removing one is no redraw: allowed
    with pytest.raises(_abi.QuadGymError, match="already bound"):
        _cur(env, R.ONE)
    assert lib.qg_walk_destroy(env._walk._h) == -1 and b"qg_cmdcur_destroy first" in lib.qg_last_error()
    # the resident step mode cannot be on under a curriculum: a simulator with a walking layer bound refuses to start it
    mail_a, mail_p = torch.zeros((2, n, 12), device=DEV), torch.zeros((2, n, 35), device=DEV)
    with pytest.raises(_abi.QuadGymError, match="walking task layer"):
        env._sim.resident_start(mail_a, mail_p)
    torch.cuda.synchronize()
    assert np.array_equal(cur.state(), s0) and np.array_equal(env._walk.state(), w0)       # nothing was launched on the way
    cur.close()
    env._walk.set_command_sampler(sampler)                    # unbound again: the sampler goes in, and then a curriculum is refused
    with pytest.raises(_abi.QuadGymError, match="command sampler installed"):
        _cur(env, R.MAIN)
    assert lib.qg_walk_set_command_sampler(env._walk._h, None) == 0
    again = _cur(env, R.MAIN)                                 # and a new one binds where the first was destroyed
    assert np.array_equal(again.state(), s0)
    env.close()
    assert again._h is None and env._sim is None


# ---- 6. the wrapper in stacks ------------------------------------------------------------------------------------------------------------------
CRITERIA = {"progress_direction_reward_local": (1, 0.0), "control_cost": (-1, 0.0)}
OPTIONS = dict(speed=(0.0, 0.6), bins=(3, 4), initial_speed=(0.0, 0.2), criteria=CRITERIA, weight_max=8, delta=3, resample_steps=5, min_steps=2,
               seed=3)
STACKS = {
    "alone": lambda env: DeviceCommandCurriculumVecEnv(env, **OPTIONS),
    "normalize_outside": lambda env: DeviceVecNormalize(DeviceCommandCurriculumVecEnv(env, **OPTIONS)),
    "normalize_inside": lambda env: DeviceCommandCurriculumVecEnv(DeviceVecNormalize(env), **OPTIONS),
    "gait_outside": lambda env: DeviceGaitRewardVecEnv(DeviceCommandCurriculumVecEnv(env, **OPTIONS), weights={"feet_air_time": 1.0}),
    "gait_inside": lambda env: DeviceCommandCurriculumVecEnv(DeviceGaitRewardVecEnv(env, weights={"feet_air_time": 1.0}),
                                                             **dict(OPTIONS, criteria=dict(CRITERIA, flight=(-1, 10.0)))),
}


def _layer(stack):
    while not isinstance(stack, DeviceCommandCurriculumVecEnv):
        stack = stack.venv
    return stack


@pytest.mark.parametrize("kind", ["walking", "po"])
@pytest.mark.parametrize("order", sorted(STACKS))
def test_wrapper_in_stacks_through_episode_ends_with_snapshot_and_restore(kind, order):
    n = 64
    make = (lambda: WalkingQuadrupedVecEnv(n, nan_direction=False, max_time=0.05)) if kind == "walking" else \
           (lambda: POWalkingQuadrupedVecEnv(n, obs_window=2, nan_direction=False, max_time=0.05))
    stack = STACKS[order](make())
    layer = _layer(stack)
    po = kind == "po"
    D = stack.obs_dim
    stack.reset()
    assert layer.curriculum.bins()["segment"].tolist() == [1] * n                  # reset began a new segment everywhere
    gen = torch.Generator(device=DEV).manual_seed(9)
    acts = torch.rand((12, n, 12), generator=gen, device=DEV) * 2 - 1

    def run(lo, hi, with_components):
        rows = []
        for t in range(lo, hi):
            obs, rew, done = torch.zeros((n, D), device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV)
            kw = dict(terminal_obs=torch.zeros((n, D), device=DEV)) if po else {}
            if with_components:
                kw["components"] = torch.zeros((n, len(stack.reward_keys)), device=DEV)
            assert stack.step_tensor(acts[t], obs, rew, done, **kw) is None
            torch.cuda.synchronize()
            velocity, heading = layer.commands()
            assert _same(layer.commands_tensor.cpu().numpy(), np.concatenate([velocity, heading], axis=1))
            rows.append(b"".join(x.cpu().numpy().tobytes() for x in (obs, rew, done, layer.commands_tensor)) + layer.curriculum.state().tobytes())
        return rows

    run(0, 4, False)                                          # the wrapper's own component rows where the caller passes none
    snap = stack.snapshot()
    first = run(4, 10, True)
    stats = layer.curriculum.stats()
    assert stats["episodes"].sum() >= n and (layer.curriculum.weights() > 0).sum() > 4    # episodes ended, and the grid moved outward
    stack.restore(snap)
    assert _same(layer.commands_tensor.cpu().numpy(), np.concatenate(layer.commands(), axis=1))
    assert run(4, 10, True) == first
    # the NumPy cold path runs the same launches
    obs, rew, done, infos = stack.step(acts[10].cpu().numpy())
    assert obs.shape == (n, D) and rew.shape == (n,) and len(infos) == n
    stack.close()
    assert layer.curriculum._h is None
