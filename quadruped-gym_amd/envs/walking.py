"""Walking task envs on the device task layer (``qg_walk_*`` in ``include/quadgym.h``): the batched
counterpart of the reference's ``WalkingQuadrupedEnv`` (``src/envs/walking_quad.py``) -- velocity / heading
command, settling-time action mask, control-signal frequency / amplitude estimator, the 11-term
``input_control_reward`` and the flip + time-limit terminations -- for N robots per kernel launch.
"""
from __future__ import annotations

import numpy as np

from .. import _abi
from ..model.loader import load_model
from ..sim import BatchedSim
from ..task_layers import ObsPack, WalkLayer, default_walk_params  # noqa: F401  (default_walk_params: re-exported)
from .infos import LazyInfos, finished_only_infos
from .vec_env import BatchedEnvBase, _VecEnvBase

REWARD_KEYS = ["alive_bonus", "control_cost", "progress_direction_reward_local", "progress_speed_cost_local",
               "heading_reward", "orientation_reward", "body_height_cost", "joint_posture_cost",
               "control_amplitude_cost", "control_frequency_cost", "diff_ideal_position_cost"]   # walking_quad.py:332-351


def sample_command(options=None, uniform=None):
    """``VelocityHeadingControls.sample`` (``src/envs/control_inputs.py:74-115``): returns
    ``(velocity_xy, heading_xy)``; draws from ``np.random.uniform`` in the reference's order."""
    uniform = uniform or np.random.uniform
    options = options or {}
    lo, hi = options.get("min_speed", 0.0), options.get("max_speed", 1.0)
    th = options.get("fixed_heading_angle")
    theta = th if th is not None else uniform(-np.pi, np.pi)
    al = options.get("fixed_velocity_angle")
    alpha = al if al is not None else uniform(-np.pi, np.pi)
    sp = options.get("fixed_speed")
    speed = sp if sp is not None else uniform(lo, hi)
    return (speed * np.cos(alpha), speed * np.sin(alpha)), (np.cos(theta), np.sin(theta))


def _component_infos(n, comps, extra, mode="lazy"):
    """``infos`` of a walking step: per env the reward-component dict the reference returns as ``info`` (walking_quad.py:419), plus
    the SB3 entries of the envs in ``extra``; built on first access (see envs/infos.py), or -- ``mode="finished"`` -- only for the
    envs that finished."""
    def make(i):
        d = dict(zip(REWARD_KEYS, comps[i].tolist()))
        e = extra.get(i)
        if e:
            d.update(e)
        return d
    if mode == "finished":
        return finished_only_infos(n, {i: make(i) for i in extra})
    return LazyInfos(n, make)


class WalkingQuadrupedVecEnv(BatchedEnvBase, _VecEnvBase):      # SB3's VecEnv where importable (what `PPO(..., env)` checks for), else object
    """N walking robots; SB3 VecEnv calling convention (replaces ``SubprocVecEnv([make_env]*N)`` at
    ``src/train_quadruped.py:50``).  ``infos[i]`` is the reward-component dict the reference returns as
    ``info`` (``walking_quad.py:146-148,419``), which ``RewardCallback`` reads (``train_quadruped.py:86-97``)."""

    reward_keys = REWARD_KEYS
    _infos_mode_error = ("infos_mode must be 'lazy' (every env's component dict, built when touched) or 'finished' (content "
                         "for the envs that finished only; `last_components` holds every env's components as one array)")

    def __init__(self, num_envs, settling_time=0, random_controls=False, random_init=False, reset_options=None,
                 model_path="builtin", max_time=10.0, frame_skip=4, device=0, env_index_base=0, seed=0, walk_params=None,
                 device_commands=False, auto_reset=True, use_default_termination=True, infos_mode="lazy", nan_direction=True,
                 dynamics_randomization=None, push_randomization=None):
        qg_model = self._init_common(num_envs, load_model(model_path), max_time, frame_skip, infos_mode, seed)
        self.random_controls, self.random_init, self.reset_options = random_controls, random_init, reset_options
        task = _abi.default_task()
        task.frame_skip = self.frame_skip
        task.max_time = self.max_time
        task.use_time_limit = 1 if use_default_termination else 0   # quadruped.py:52,99-100
        task.use_fall = 0
        task.use_flip = 1                                   # walking_quad.py:156-166
        # VecEnv semantics: finished envs restart inside the step.  The single-robot facades switch it off: there the caller
        # resets, as with the reference's env (a finished robot left alone keeps reporting `terminated`)
        self.auto_reset = bool(auto_reset)
        task.auto_reset = 1 if self.auto_reset else 0
        task.reset_flags = _abi.RESET_RANDOM_YAW if random_init else 0     # walking_quad.py:68-75,118-119
        if dynamics_randomization is not None:      # a new dynamics row per env at every reset and auto-reset
            task.reset_flags |= _abi.RESET_DYNAMICS
        self._make_sim(task, qg_model, device, env_index_base, dynamics_randomization, push_randomization, BatchedSim)
        self.params = walk_params if walk_params is not None else default_walk_params()
        self.params.settling_time = float(settling_time)
        # nan_direction=True is the reference: unit() of an exactly zero local velocity (or command) is NaN and so are the direction
        # term and the reward of that step (math_utils.py:7-8, walking_quad.py:197-205).  In this f32 pipeline the local xy velocity is
        # EXACTLY zero on the first step of every episode, so a training run wants False: the term is 0 there.
        self.nan_direction = bool(nan_direction)
        if not self.nan_direction:
            self.params.unit_zero = 1
        self._walk = WalkLayer(self._sim, self.params)
        self._flags = task.reset_flags
        # random_controls (walking_quad.py:121-122).  device_commands=False: commands are redrawn on the host with
        # np.random.uniform in the reference's order (VelocityHeadingControls.sample); True: on the GPU, inside reset and
        # the step's auto-reset, from the env's own counter-based stream -- rollouts through step_tensor never touch the host.
        self.device_commands = bool(device_commands) and bool(random_controls)
        if self.device_commands:
            self._walk.set_command_sampler(_abi.QgCommandSampler.from_options(reset_options))
        self._init_spaces(self._walk.obs_dim)
        self.velocity = np.zeros((self.num_envs, 2), np.float32)
        self.heading = np.zeros((self.num_envs, 2), np.float32)
        self.dt = qg_model.timestep * self.frame_skip

    # -- commands ---------------------------------------------------------------------------------
    def set_commands(self, velocity_xy, heading_xy):
        self.velocity[:] = np.asarray(velocity_xy, np.float32).reshape(self.num_envs, 2)
        self.heading[:] = np.asarray(heading_xy, np.float32).reshape(self.num_envs, 2)
        self._walk.set_commands(self.velocity, self.heading)

    def commands(self):
        """``(velocity_xy, heading_xy)`` as they stand on the device, ``[num_envs, 2]`` each."""
        self._walk.get_commands(self.velocity, self.heading)
        return self.velocity, self.heading

    def estimates(self):
        return self._walk.estimates()

    # -- checkpoint / resume (the reference resumes the policy only, train_quadruped.py:114-141) -------------------
    def snapshot(self):
        """Everything this env keeps per robot -- physics state, reset streams, the walking layer's task state (estimator included)
        and, for the partially observable env, the filter estimate and the frame ring -- as a ``dict`` of NumPy arrays.
        ``restore(snapshot)`` on an env of the same shape continues bit for bit."""
        return dict(super().snapshot(), walk=self._walk.state(), velocity=self.velocity.copy(), heading=self.heading.copy())

    def _check_snapshot(self, snap):
        """Raises unless every part of ``snap`` fits this env; writes nothing."""
        self._walk.check_state(snap["walk"])
        super()._check_snapshot(snap)
        if np.asarray(snap["velocity"]).shape != self.velocity.shape or np.asarray(snap["heading"]).shape != self.heading.shape:
            raise ValueError("the snapshot's commands do not fit this env")

    def restore(self, snap):
        """All-or-nothing: every part of the snapshot is checked against this env BEFORE anything is written.  Continues bit for
        bit with ``device_commands=True`` (or fixed commands); with host-side command sampling the commands an auto-reset re-draws
        come from NumPy's global generator, which a snapshot does not hold."""
        super().restore(snap)             # checks every part, the subclasses' too, before it writes
        self._walk.load_state(snap["walk"])
        self.velocity[:], self.heading[:] = snap["velocity"], snap["heading"]

    def _resample(self, idx):
        if self.device_commands:          # already redrawn on the device by the reset / auto-reset itself
            return
        for i in idx:
            v, hd = sample_command(self.reset_options)
            self.velocity[i], self.heading[i] = v, hd
        self._walk.set_commands(self.velocity, self.heading)

    # -- VecEnv protocol ------------------------------------------------------------------------------
    _zero_finished = True                 # a finished env's row of the step is its terminal observation; its reset observation is zeros

    def _layer_reset(self):
        self._walk.reset(self._seed, self._flags)
        return np.zeros((self.num_envs, 33), np.float32)

    def _layer_step(self):
        """``(obs, reward, done, components, terminal)``: ``terminal[i]`` is what env ``i`` ended with, if it finished."""
        obs, rew, done, comps = self._walk.step(self._actions)
        return obs, rew, done, comps, obs

    def reset(self):
        obs = self._layer_reset()
        self._reset_contact()
        if self.random_controls:                              # walking_quad.py:121-122
            self._resample(range(self.num_envs))
        return obs

    def step_wait(self):
        obs, rew, done, comps, term = self._layer_step()
        dones = done.astype(bool)
        finished = np.nonzero(dones)[0] if self.auto_reset else ()
        extra = {int(i): {"terminal_observation": term[i].copy(), "TimeLimit.truncated": False} for i in finished}
        infos = _component_infos(self.num_envs, comps, extra, self.infos_mode)
        if len(finished):
            if self._zero_finished:
                obs = obs.copy()
                obs[dones] = 0.0
            if self.random_controls:
                self._resample(finished)
        self.last_components = comps
        return obs, rew, dones, infos

    def step_tensor(self, actions, obs, reward, done, components=None, stream=None):
        """Zero-copy step on CUDA tensors of this env's device, contiguous: float32 ``[N,12]``, ``[N,33]``, ``[N]``, uint8 (or bool)
        ``[N]``, ``[N,11]``.  Anything else raises ``ValueError`` before the launch."""
        self._walk.step_device(actions, obs, reward, done, components, stream)

    def close(self):
        super().close()
        self._walk = None


def _facade_kwargs(kwargs, allowed):
    """Keyword arguments the reference forwards to ``QuadrupedEnv.__init__`` (``walking_quad.py:11-12``).  The rendering ones
    are accepted when they ask for nothing; ``reward_fns`` / ``termination_fns`` would REPLACE the task's reward and
    terminations in the reference (``quadruped.py:97-100``) -- the device task layer cannot honour that, so it refuses
    instead of silently running the built-in walking reward."""
    display = {"render_mode", "width", "height", "render_fps", "save_video", "video_path"}
    extra = set(kwargs) - allowed - display - {"reward_fns", "termination_fns"}
    if extra:
        raise TypeError(f"unexpected keyword arguments {sorted(extra)}")
    if kwargs.get("render_mode") is not None or kwargs.get("save_video"):
        raise NotImplementedError("rendering / video recording is not part of the HIP path")
    for key in ("reward_fns", "termination_fns"):
        if kwargs.get(key) is not None:
            raise NotImplementedError(f"{key}: the walking task layer evaluates the reference's input_control_reward and flip / "
                                      "time-limit terminations on the device; custom callables run through QuadrupedEnv / "
                                      "QuadrupedVecEnv")
    args = {k: v for k, v in kwargs.items() if k in allowed}
    args.setdefault("model_path", "./models/quadruped/scene.xml")      # quadruped.py:41
    return args


class _SingleRobotFacade:
    """The reference's single-robot calling convention over a batched env of one robot without auto-reset (``self._vec``)."""

    reward_keys = REWARD_KEYS

    def _wrap(self, vec):
        self._vec = vec
        self.action_space, self.observation_space = vec.action_space, vec.observation_space
        self.model = vec.model
        self.info = {}

    def reset(self, seed=None, options=None):
        if options is not None:
            self._vec.reset_options = options                  # walking_quad.py:100-101
        obs = self._vec.reset()
        self.info = {}
        return obs[0].astype(np.float64), self.info

    def step(self, action):
        obs, rew, dones, infos = self._vec.step(np.asarray(action, np.float32)[None])
        self.info = dict(infos[0])                             # walking_quad.py:146-148: info = the component dict
        return obs[0].astype(np.float64), float(rew[0]), bool(dones[0]), False, self.info

    def close(self):
        self._vec.close()


class WalkingQuadrupedEnv(_SingleRobotFacade):
    """One walking robot with the reference's constructor (``walking_quad.py:11``): ``settling_time``,
    ``random_controls``, ``random_init``, ``reset_options`` plus the base env's keyword arguments;
    ``step`` returns ``(obs, reward, terminated, False, info)`` with ``info`` = the component dict."""

    def __init__(self, settling_time=0, random_controls=False, random_init=False, reset_options=None, **kwargs):
        args = _facade_kwargs(kwargs, {"model_path", "max_time", "frame_skip", "device", "use_default_termination"})
        self._wrap(WalkingQuadrupedVecEnv(1, settling_time, random_controls, random_init, reset_options, auto_reset=False, **args))

    def set_command(self, velocity_xy, heading_xy):
        self._vec.set_commands([velocity_xy], [heading_xy])


class POWalkingQuadrupedVecEnv(WalkingQuadrupedVecEnv):
    """Batched ``POWalkingQuadrupedEnv`` (``src/envs/po_walking_quad.py``): the observation is the stack of the last
    ``obs_window`` 26-value frames [gyro, accel, Madgwick-IMU Euler angles, body_vel xy, data.ctrl, command vx vy theta]
    (``:48-56``); rewards and terminations are the walking task's."""

    FRAME = 26
    _zero_finished = False                # a finished env's row of the step already holds its reset stack

    def __init__(self, num_envs, obs_window=1, **kwargs):
        super().__init__(num_envs, **kwargs)
        self._obs_pack = ObsPack(self._walk, obs_window)
        self.obs_window = self._obs_pack.obs_window
        self._init_spaces(self._obs_pack.obs_dim)              # po_walking_quad.py:27

    def _layer_reset(self):
        return self._obs_pack.reset(self._seed, self._flags)

    def _layer_step(self):
        return self._obs_pack.step(self._actions)

    def snapshot(self):
        snap = super().snapshot()
        snap["po"] = self._obs_pack.state()
        return snap

    def _check_snapshot(self, snap):
        super()._check_snapshot(snap)
        if "po" not in snap:
            raise ValueError("the snapshot holds no observation-pack state (it was taken from an env without one)")
        self._obs_pack.check_state(snap["po"])

    def restore(self, snap):
        super().restore(snap)             # checks every part, "po" included, before it writes
        self._obs_pack.load_state(snap["po"])

    def step_tensor(self, actions, obs, reward, done, components=None, terminal_obs=None, stream=None):
        """Zero-copy step on CUDA tensors: ``actions`` float32 ``[N,12]`` -> ``obs`` float32 ``[N, 26 * obs_window]`` (the
        stacked frames; rows of envs that finished already hold the reset stack), ``reward`` ``[N]``, ``done`` uint8 (or bool)
        ``[N]``, optionally ``components`` ``[N,11]`` and ``terminal_obs`` (the stack each finished env ended with).  All on this
        env's device and contiguous; anything else raises ``ValueError`` before the launch."""
        self._obs_pack.step_device(actions, obs, reward, done, components, terminal_obs, stream)

    def close(self):
        super().close()
        self._obs_pack = None


class POWalkingQuadrupedEnv(_SingleRobotFacade):
    """One robot with the reference's constructor ``POWalkingQuadrupedEnv(obs_window=1, **kwargs)``
    (``po_walking_quad.py:10``; ``train_quadruped.py:16-22`` builds it with ``obs_window=10``)."""

    def __init__(self, obs_window=1, **kwargs):
        args = _facade_kwargs(kwargs, {"settling_time", "random_controls", "random_init", "reset_options", "model_path", "max_time",
                                       "frame_skip", "device", "use_default_termination"})
        self._wrap(POWalkingQuadrupedVecEnv(1, obs_window=obs_window, auto_reset=False, **args))
        self.obs_window = obs_window

