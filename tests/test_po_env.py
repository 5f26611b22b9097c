"""The partially observable pack (qg_po_*) against oracle/po_oracle.py.  The Madgwick filter of the
reference comes from the `ahrs` package, which is not available offline: the oracle restates the published
algorithm -- parity unpinned, stated here.

Two kinds of check.  test_po_frames_match_oracle drives the oracle with the GPU's OWN sensor values: it pins what the pack computes
(the filter's Euler angles, the settling gate, the FIFO, terminal and reset stacks) and, for the pass-through columns, only their
place.  test_po_rollout_frames_match_oracle_driven_from_the_state pins the pass-through columns themselves -- gyro, accelerometer,
body velocity, data.ctrl, command -- over rollouts with auto-resets: at every step the composed checker (tests/po_step_reference.py:
settling gate and clip -> f64 physics oracle -> frame) is restarted from the device's STATE and takes none of its sensors.
tests/test_kernel_leaves_gpu.py holds the whole stack of every fused PO instantiation to the same checker over one and two steps."""
import numpy as np
import pytest

from oracle import po_oracle as P

import po_step_reference as R


def test_madgwick_restatement_properties():
    # unit output, no update for an exactly zero gyro, accelerometer pulls the estimate towards gravity
    q = np.array([0.9, 0.1, -0.2, 0.3]); q /= np.linalg.norm(q)
    assert np.array_equal(P.madgwick_update_imu(q, [0, 0, 0], [0, 0, 9.8], 0.02), q)
    q1 = P.madgwick_update_imu(q, [0.3, -0.2, 0.1], [0.1, 0.2, 9.7], 0.02)
    assert abs(np.linalg.norm(q1) - 1) < 1e-15
    # pure gyro integration when the accelerometer reads zero: dq = 0.5 q (x) w dt
    q2 = P.madgwick_update_imu([1, 0, 0, 0], [0, 0, 1.0], [0, 0, 0], 0.01)
    assert np.allclose(q2, np.array([1, 0, 0, 0.005]) / np.linalg.norm([1, 0, 0, 0.005]))
    q = np.array([1.0, 0, 0, 0])
    for _ in range(5000):
        q = P.madgwick_update_imu(q, [1e-9, 0, 0], [0, 0.5, 9.8], 0.02)
    assert P.to_angles(q)[0] == pytest.approx(np.arctan2(0.5, 9.8), abs=2e-3)
    assert np.allclose(P.to_angles([np.cos(0.35), 0, 0, np.sin(0.35)]), [0, 0, 0.7])


@pytest.mark.gpu
@pytest.mark.parametrize("window,settle", [(1, 0.0), (4, 0.08), (10, 0.5)])
def test_po_frames_match_oracle(window, settle):
    """The stacked observation against oracle/po_oracle.py at frame_skip 10; (window, settle) = (10, 0.5) is the reference's training
    setting (src/train_quadruped.py:16-19: obs_window 10, frame_skip 10, settling_time 0.5).
    What this test does and does not check: the oracle is fed the GPU's OWN frame for the gyro, accelerometer, body-velocity and
    data.ctrl columns (0-5, 9-10, 11-22 of a frame) -- those are pass-through values here (the physics behind them is checked in
    test_po_rollout_frames_match_oracle_driven_from_the_state below and, per fused instantiation, in tests/test_kernel_leaves_gpu.py),
    so for them the comparison only proves that they sit at the right place of the right frame of the stack.  The columns the observation pack COMPUTES are the real checks: the Madgwick-IMU Euler angles (6-8; filter update, the
    settling-time gate on the f64 clock, the aliasing of the estimate with data.qpos after a reset), the command columns (23-25: the
    command in force, its heading angle), the FIFO order over `window` frames, and the terminal / reset stacks at auto-resets."""
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
    n, fs = 40, 10
    env = POWalkingQuadrupedVecEnv(n, obs_window=window, settling_time=settle, frame_skip=fs, max_time=0.6, random_init=True,
                                   random_controls=True, reset_options={"min_speed": 0.1, "max_speed": 0.4})
    assert env.observation_space.shape == (26 * window,)                       # po_walking_quad.py:21-27
    dt = 0.002 * fs
    o = P.POOracle(n, dt, settle, window)
    default_ctrl = np.array([0, 0, -0.5] * 4, float)
    np.random.seed(5)
    zero_cmd_v, zero_cmd_h = np.zeros(2), np.zeros(2)
    obs = env.reset()
    # first reset: estimate [1,0,0,0], commands still zero when the observation is taken (:59-69, control_inputs.py:9-12)
    for i in range(n):
        exp = o.reset_env(i, default_ctrl, np.array([1.0, 0, 0, 0]), zero_cmd_v, zero_cmd_h)
        assert np.allclose(obs[i], exp, atol=1e-6)
    vel, head = env.velocity.copy(), env.heading.copy()
    rng = np.random.default_rng(1)
    t = np.zeros(n)
    saw_done = False
    for k in range(70):
        a = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
        obs, rew, dones, infos = env.step(a)
        qquat = env._sim.get_state()[0][:, 3:7].astype(np.float64)
        for _ in range(fs):                       # the engine's clock: one f64 addition per substep
            t += 0.002
        for i in range(n):
            stacked = infos[i]["terminal_observation"] if dones[i] else obs[i]
            fr = stacked[-26:].astype(np.float64)
            sens = np.zeros(33); sens[15:18] = fr[0:3]; sens[12:15] = fr[3:6]; sens[30:32] = fr[9:11]
            # while the estimate aliases qpos, the kernel reads the post-step quaternion; an env that finished has been
            # reset already, so skip the (rare) aliasing + termination combination
            exp = o.step_env(i, t[i], sens, fr[11:23], qquat[i], vel[i], head[i])
            if not (dones[i] and o.alias[i]):
                assert np.allclose(stacked, exp, rtol=2e-4, atol=2e-4), (k, i)
            if dones[i]:
                saw_done = True
                # reset frame: previous estimate, default ctrl, the command of the episode that just ended
                exp = o.reset_env(i, default_ctrl, np.array([1.0, 0, 0, 0]), vel[i], head[i])
                assert np.allclose(obs[i], exp, rtol=2e-4, atol=2e-4), (k, i)
                t[i] = 0.0
        vel, head = env.velocity.copy(), env.heading.copy()                  # commands re-sampled after the step
    assert saw_done
    env.close()


def _link_grid_plus_one():
    from kernel_leaves import link_max
    from parity import simds
    return link_max(simds()) + 1


@pytest.mark.gpu
@pytest.mark.parametrize("size,window,settle,steps", [("small", 10, 0.0, 40), ("small", 10, 0.08, 40), ("first_quad", 4, 0.08, 12)])
def test_po_rollout_frames_match_oracle_driven_from_the_state(oracle, size, window, settle, steps):
    """The pass-through columns of the newest frame -- gyro 0-2, accelerometer 3-5, body velocity 9-10, data.ctrl 11-22, command 23-25
    -- against the composed checker driven from the device's STATE, not from its sensors: before every env-step the state is read, and
    the checker (tests/po_step_reference.py) gates and clips the action on the f64 clock of that state's step counter, steps the f64
    physics oracle from that state and lays its sensors out as a frame with the command in force.  A finished env is compared through
    the newest frame of its terminal stack.  Tolerances: TOL["A"] of tests/parity.py (one env-step at frame_skip 4 from an
    identical f32 state: obs for gyro and body velocity, accel for the accelerometer), 1e-6 for ctrl and command (exact values in
    f32).  Every (env, step) is compared, none is left out: the columns compared do not pass through the orientation estimate, so the
    estimate aliasing qpos at a termination (what test_po_frames_match_oracle skips) does not matter here.  The angle columns keep
    their check in test_po_frames_match_oracle.
    n = 40: 2.5 workgroups of the link kernel, 40 steps at max_time 0.12 s = 15 env-steps per episode: every env passes two
    auto-resets (random yaw, re-drawn commands), with and without the settling gate.  The third case is the first quad grid -- one
    env more than the link kernel serves, the last workgroup holding ONE env -- on a seeded sample of 256 envs plus the last 16;
    its 12 steps end before the time limit, and the settling gate opens after the tenth."""
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
    from parity import TOL
    n = 40 if size == "small" else _link_grid_plus_one()
    fs = 4
    env = POWalkingQuadrupedVecEnv(n, obs_window=window, settling_time=settle, frame_skip=fs, max_time=0.12, random_init=True,
                                   random_controls=True)
    sim = env._sim
    model, task = sim.model, sim.get_task()
    assert task.frame_skip == fs and task.sensor_lag == 1
    pick = np.arange(n) if n <= 272 else np.unique(np.r_[np.random.default_rng(7).choice(n - 16, 256, replace=False), np.arange(n - 16, n)])
    np.random.seed(6)
    env.reset()
    rng = np.random.default_rng(3)
    maxima, compared, finished, resets = {}, 0, 0, np.zeros(n, int)
    for k in range(steps):
        a = rng.uniform(-1.2, 1.2, (n, 12)).astype(np.float32)
        q, v, act, _, ns = sim.get_state()
        vel, head = env.velocity.copy(), env.heading.copy()                  # the command in force: re-drawn after the step
        obs, rew, dones, infos = env.step(a)
        applied, ctrl = R.gated_control(ns[pick], a[pick], settle)
        out = R.physics(oracle, model, task, (q[pick], v[pick], act[pick], ns[pick]), applied)
        exp = R.frame_columns(out["sens"], ctrl, vel[pick], head[pick])
        got = np.stack([(infos[i]["terminal_observation"] if dones[i] else obs[i])[-26:] for i in pick])
        R.compare_newest(got, exp, TOL["A"], 0.002 * fs, what="newest", angles=False, rows=pick, maxima=maxima)
        compared += len(pick)
        finished += int(dones[pick].sum())
        resets += dones
    assert compared == len(pick) * steps
    if size == "small":
        assert finished > 0 and resets.min() >= 2
    R.record("QG_PO_PARITY_OUT", f"rollout n={n} window={window} settle={settle} steps={steps} compared={compared} finished={finished}: "
             + R.format_maxima(maxima))
    env.close()


@pytest.mark.gpu
def test_po_single_env_facade():
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedEnv
    env = POWalkingQuadrupedEnv(obs_window=10, model_path="builtin", max_time=20, frame_skip=10, settling_time=0.5, random_controls=True,
                                reset_options={"fixed_heading_angle": 0.0, "fixed_velocity_angle": 0.0, "fixed_speed": 0.3})   # train_quadruped.py:16-46
    obs, info = env.reset()
    assert obs.shape == (260,) and env.observation_space.shape == (260,)         # train_quadruped.py:19: 26 x 10
    obs, r, term, trunc, info = env.step(np.zeros(12, np.float32))
    assert obs.shape == (260,) and np.allclose(obs[-15:-3], [0, 0, -0.5] * 4)    # settling: joint centres applied
    assert np.allclose(obs[-3:], [0.3, 0.0, 0.0], atol=1e-6)
    env.close()


@pytest.mark.gpu
def test_po_frames_show_the_command_in_force_with_device_sampler():
    """po_walking_quad.py:48-69 with commands redrawn on the device: the terminal frame and the reset frame of an episode
    still show the command that was in force (the reference builds both before ``control_inputs.sample`` runs,
    walking_quad.py:103,121-122); the first frame of the next episode shows the new one."""
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
    n = 16
    env = POWalkingQuadrupedVecEnv(n, obs_window=1, max_time=0.016, random_controls=True, device_commands=True, seed=3,
                                   reset_options={"min_speed": 0.5, "max_speed": 1.5})
    first = env.reset()
    assert not first[:, 23:26].any()                      # nothing had been drawn when the reset frame was built
    v0, h0 = (x.copy() for x in env.commands())
    assert (np.linalg.norm(v0, axis=1) >= 0.5 - 1e-6).all()
    a = np.zeros((n, 12), np.float32)
    o1 = env.step(a)[0]
    assert np.allclose(o1[:, 23:25], v0, atol=1e-6) and np.allclose(o1[:, 25], np.arctan2(h0[:, 1], h0[:, 0]), atol=1e-5)
    o2, _, dones, infos = env.step(a)                     # 8 substeps: episode over, auto-reset, new command drawn
    assert dones.all()
    term = np.stack([i["terminal_observation"] for i in infos])
    assert np.allclose(term[:, 23:25], v0, atol=1e-6)     # terminal frame: old command
    assert np.allclose(o2[:, 23:25], v0, atol=1e-6)       # reset frame: still the old command (reference quirk)
    v1, h1 = (x.copy() for x in env.commands())
    assert np.abs(v1 - v0).max() > 1e-3
    o3 = env.step(a)[0]
    assert np.allclose(o3[:, 23:25], v1, atol=1e-6) and np.allclose(o3[:, 25], np.arctan2(h1[:, 1], h1[:, 0]), atol=1e-5)
    env.close()


@pytest.mark.gpu
def test_po_step_tensor_equals_host_step():
    """The zero-copy entry point (device tensors, caller's stream) returns what the NumPy path returns."""
    import torch
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
    n, w = 24, 3
    a_env = POWalkingQuadrupedVecEnv(n, obs_window=w, max_time=0.05)
    b_env = POWalkingQuadrupedVecEnv(n, obs_window=w, max_time=0.05)
    a_env.reset(); b_env.reset()
    v = np.tile([[0.3, 0.1]], (n, 1)); h = np.tile([[1.0, 0.0]], (n, 1))
    a_env.set_commands(v, h); b_env.set_commands(v, h)
    dev = torch.device("cuda:0")
    obs = torch.empty((n, 26 * w), device=dev); rew = torch.empty(n, device=dev)
    done = torch.empty(n, device=dev, dtype=torch.uint8); comps = torch.empty((n, 11), device=dev); term = torch.empty((n, 26 * w), device=dev)
    rng = np.random.default_rng(4)
    for k in range(9):                                      # crosses the 0.05 s time limit: auto-reset inside the step
        a = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
        o, r, d, infos = a_env.step(a)
        b_env.step_tensor(torch.from_numpy(a).to(dev), obs, rew, done, comps, term)
        torch.cuda.synchronize()
        assert np.array_equal(o, obs.cpu().numpy()) and np.array_equal(r, rew.cpu().numpy(), equal_nan=True)
        assert np.array_equal(d, done.cpu().numpy().astype(bool))
        for i in np.nonzero(d)[0]:
            assert np.array_equal(infos[i]["terminal_observation"], term[i].cpu().numpy())
    a_env.close(); b_env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("window,modified,n", [(1, False, 40), (4, False, 40), (10, False, 40), (12, False, 40), (64, False, 40), (10, True, 40),
                                                (10, False, 4096),
                                                # round 3: the wave-level fused forms above 4096 envs -- one leg per lane with one and two waves
                                                # per SIMD (8192 / 40 000 envs), two legs per lane (20 000 / 32 768), tables in LDS (5000, modified
                                                # robot); windows whose history is and is not a multiple of 16 bytes, a ragged last wave
                                                (4, False, 8192), (10, False, 20000), (10, False, 32768), (12, False, 40000), (10, True, 5000),
                                                (1, False, 20001), (64, False, 6001), (2, False, 16389),
                                                # round 4: windows whose last copy batch reads past the lane's share of the row (8, 13: the
                                                # frame ring's slack), on the in-loop copy of the one-leg-per-lane kernel at two waves per
                                                # SIMD and of the two-legs-per-lane kernel
                                                (8, False, 16400), (13, False, 40001), (13, False, 20000)])
def test_po_fused_launch_equals_separate_launches(window, modified, n, monkeypatch):
    """The whole partially observable step is ONE launch at every batch size AUTO serves: physics + walking task layer + observation
    pack in qg_step_kernel_link<WALK, PO> up to 4096 envs and (round 3) in qg_step_kernel_quad / _pair<.., WALK, PO> above;
    QG_PO_UNFUSED=1 at construction keeps the observation pack a launch of its own.  Same arithmetic, same order: physics,
    terminations, re-drawn commands AND rewards must agree to the bit (the reward function is compiled without multiply-add
    contraction since round 4: round 3's helper waves had moved its evaluation into another kernel role and the two roles contracted
    a*b + c*d differently); the frames to the last bits of the filter's Euler angles (the filter is still contracted per kernel)."""
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
    fs = 4                                                         # n = 40: 2.5 workgroups of the fused kernel; 4096: the full grid
    kw = dict(obs_window=window, settling_time=0.05, frame_skip=fs, max_time=0.12, random_init=True, random_controls=True,
              device_commands=True, seed=11, reset_options={"min_speed": 0.1, "max_speed": 0.4})
    import quadruped_gym_amd.envs.walking as W
    orig = W.load_model

    def tweaked(path):                                             # a heavier, weaker robot: the kernel variant with tables in LDS
        m, layout = orig(path)
        for k in range(4):
            m.body_mass[3 + 3 * k] *= 1.25
            m.act_kp[1 + 3 * k] = 85.0
        return m, layout
    if modified:
        monkeypatch.setattr(W, "load_model", tweaked)
    fused = POWalkingQuadrupedVecEnv(n, **kw)
    monkeypatch.setenv("QG_PO_UNFUSED", "1")
    split = POWalkingQuadrupedVecEnv(n, **kw)
    monkeypatch.delenv("QG_PO_UNFUSED")
    assert fused._sim.baked == (not modified)
    assert np.array_equal(fused.reset(), split.reset())
    rng = np.random.default_rng(2)
    finished, worst = 0, 0.0
    for k in range(50 if n <= 8192 else 34):                       # 15 env-steps per episode: three (two) auto-resets per env
        a = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
        o1, r1, d1, i1 = fused.step(a)
        o2, r2, d2, i2 = split.step(a)
        assert np.array_equal(d1, d2), k
        assert np.allclose(o1, o2, rtol=0, atol=5e-6), (k, np.abs(o1 - o2).max())
        # round 4: the reward is evaluated without multiply-add contraction (walk_reward_env), so the helper wave of the walking
        # launch and the physics wave of the fused launch -- different kernels around the same function -- leave the same bits
        assert np.array_equal(r1, r2, equal_nan=True), (k, float(np.nanmax(np.abs(r1 - r2))))
        for i in np.nonzero(d1)[0]:
            assert np.allclose(i1[i]["terminal_observation"], i2[i]["terminal_observation"], rtol=0, atol=5e-6), (k, i)
        finished += int(d1.sum())
        worst = max(worst, float(np.abs(o1 - o2).max()))
        (v1, h1), (v2, h2) = fused.commands(), split.commands()
        assert np.array_equal(v1, v2) and np.array_equal(h1, h2), k
    assert finished >= 2 * n
    print(f"window {window}: largest frame difference fused vs separate {worst:.2e}")
    s1, s2 = fused._sim.get_state(), split._sim.get_state()
    for x, y in zip(s1, s2):
        assert np.array_equal(x, y)
    fused.close(); split.close()


@pytest.mark.gpu
def test_po_step_replays_from_a_hipgraph_like_eager():
    """Nothing in the fused partially observable step lives on the host between launches (ring positions, call counters, episode
    counters, command streams: all device state), so a hipGraph of env-steps can be replayed: 8 captured steps x 12 replays -- through
    auto-resets and re-drawn commands -- leave the same observations, rewards, dones and simulator state as 96 eager steps of a twin."""
    import torch
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv
    n, G = 200, 8
    kw = dict(obs_window=10, frame_skip=4, max_time=0.2, random_init=True, random_controls=True, device_commands=True, seed=5,
              reset_options={"min_speed": 0.1, "max_speed": 0.4})
    a_env, b_env = POWalkingQuadrupedVecEnv(n, **kw), POWalkingQuadrupedVecEnv(n, **kw)
    a_env.reset(); b_env.reset()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev); gen.manual_seed(9)
    acts = [torch.rand((n, 12), generator=gen, device=dev) * 2 - 1 for _ in range(G)]
    mk = lambda: (torch.empty((n, a_env.obs_dim), device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev, dtype=torch.uint8))
    obs_a, rew_a, done_a = mk()
    obs_b, rew_b, done_b = mk()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                         # one pass outside the capture (lazy initialisation), mirrored on the twin
        for g in range(G):
            a_env.step_tensor(acts[g], obs_a, rew_a, done_a, stream=side)
    torch.cuda.current_stream(dev).wait_stream(side)
    for g in range(G):
        b_env.step_tensor(acts[g], obs_b, rew_b, done_b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for g in range(G):
            a_env.step_tensor(acts[g], obs_a, rew_a, done_a, stream=torch.cuda.current_stream(dev))
    finished = 0
    for rep in range(12):                                 # 0.2 s / 8 ms = 25 steps per episode: several auto-resets
        graph.replay()
        for g in range(G):
            b_env.step_tensor(acts[g], obs_b, rew_b, done_b)
        torch.cuda.synchronize()
        assert torch.equal(obs_a, obs_b) and torch.equal(done_a, done_b), rep
        assert torch.equal(torch.nan_to_num(rew_a, nan=-1e9), torch.nan_to_num(rew_b, nan=-1e9)), rep
        finished += int(done_a.sum())
    for x, y in zip(a_env._sim.get_state(), b_env._sim.get_state()):
        assert np.array_equal(x, y)
    (v1, h1), (v2, h2) = a_env.commands(), b_env.commands()
    assert np.array_equal(v1, v2) and np.array_equal(h1, h2)
    a_env.close(); b_env.close()


def test_po_atan2_form_is_accurate_to_3e7():
    """qg_po_dev.h::po_atan2 / po_asin restated in NumPy float32 (same reduction, same Cephes polynomial, float32 arithmetic) against
    numpy's float64 arctan2 / arcsin over the plane and the unit interval: the bound the kernel comment states."""
    f = np.float32

    def po_atan2(y, x):
        y, x = y.astype(f), x.astype(f)
        ax, ay = np.abs(x), np.abs(y)
        mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = (mn * (f(1) / mx)).astype(f)
        big = a > f(0.41421356237)
        t = np.where(big, (a - f(1)) * (f(1) / (a + f(1))), a).astype(f)
        z = (t * t).astype(f)
        p = ((f(8.05374449538e-2) * z + f(-1.38776856032e-1)) * z + f(1.99777106478e-1)) * z + f(-3.33329491539e-1)
        r = ((p * z).astype(f) * t + t + np.where(big, f(0.78539816339), f(0))).astype(f)
        r = np.where(ay > ax, f(1.57079632679) - r, r)
        r = np.where(x < 0, f(3.14159265359) - r, r)
        r = np.where(mx == 0, f(0), r)
        return np.copysign(r, y).astype(f)

    rng = np.random.default_rng(0)
    ang = rng.uniform(-np.pi, np.pi, 400000)
    rad = 10.0 ** rng.uniform(-6, 6, ang.size)
    y, x = rad * np.sin(ang), rad * np.cos(ang)
    err = np.abs(po_atan2(y, x).astype(np.float64) - np.arctan2(y.astype(f).astype(np.float64), x.astype(f).astype(np.float64)))
    err = np.minimum(err, 2 * np.pi - err)                  # the branch cut at +-pi
    assert err.max() < 3e-7, err.max()
    for yy, xx in ((0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (0.0, 0.0), (1.0, 1.0), (-1.0, -1.0)):
        got = float(po_atan2(np.array([yy]), np.array([xx]))[0])
        assert abs(got - np.arctan2(yy, xx)) < 3e-7, (yy, xx, got)
    v = np.concatenate([rng.uniform(-1, 1, 200000), 1 - 10.0 ** rng.uniform(-7, -1, 50000), [-1.0, 1.0, 0.0]]).astype(f)
    s = np.sqrt(np.maximum((f(1) - v) * (f(1) + v), f(0))).astype(f)
    err = np.abs(po_atan2(v, s).astype(np.float64) - np.arcsin(v.astype(np.float64)))
    assert err.max() < 5e-7, err.max()


@pytest.mark.gpu
def test_restore_is_all_or_nothing():
    """``restore()`` checks every part of a snapshot against the env BEFORE it writes anything (round-3 advisor finding: the physics and
    the reset streams used to be overwritten before a mismatching task-layer blob was refused): a walking-only snapshot restored into a
    PO env, and a snapshot from another obs_window, are refused and leave the env exactly where it was."""
    from quadruped_gym_amd.envs.walking import POWalkingQuadrupedVecEnv, WalkingQuadrupedVecEnv
    n = 33
    kw = dict(frame_skip=4, max_time=0.2, random_init=True, random_controls=True, device_commands=True, seed=3)
    po = POWalkingQuadrupedVecEnv(n, obs_window=4, **kw)
    walk = WalkingQuadrupedVecEnv(n, **kw)
    other = POWalkingQuadrupedVecEnv(n, obs_window=6, **kw)
    rng = np.random.default_rng(0)
    for e in (po, walk, other):
        e.reset()
    for _ in range(12):
        a = rng.uniform(-1, 1, (n, 12)).astype(np.float32)
        for e in (po, walk, other):
            e.step(a)
    before = po.snapshot()
    for bad in (walk.snapshot(), other.snapshot()):
        with pytest.raises(ValueError):
            po.restore(bad)
        after = po.snapshot()
        for key in ("walk", "po", "velocity", "heading"):
            assert np.array_equal(before[key], after[key]), key
        for key in before["sim"]:
            assert np.array_equal(before["sim"][key], after["sim"][key]), key
    po.restore(before)                                   # and a matching one still goes in
    for e in (po, walk, other):
        e.close()
