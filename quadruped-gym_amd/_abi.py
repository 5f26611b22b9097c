"""ctypes mirrors of the C structs in ``include/quadgym.h`` and the loader of
``libquadgym.so`` (the HIP pipeline behind the C ABI).

There is no CPU fallback: if the shared library is missing, or no HIP device is
usable, the product path raises.
"""
from __future__ import annotations

import ctypes as C
import os

NBODY, NJNT, NQ, NV, NU, NSENSOR, MAXCP, NREWARD = 13, 12, 19, 18, 12, 33, 12, 3
OBS_FULL, OBS_IMU = 0, 1
RESET_RANDOM_YAW = 1
RESET_JOINT_JITTER = 2
RESET_DYNAMICS = 4
# per-env dynamics rows (QG_DYN_* of include/quadgym.h): column order of the [n, NDYN] arrays
NDYN = 11
DYN_COLUMNS = ("friction", "payload_mass", "payload_x", "payload_y", "payload_z", "kp_scale", "kv_scale", "force_scale",
               "damping_scale", "contact_stiffness_scale", "contact_damping_scale")
CMD_FIXED_HEADING, CMD_FIXED_VELOCITY_ANGLE, CMD_FIXED_SPEED = 1, 2, 4
MAP_AUTO, MAP_LANE, MAP_QUAD, MAP_PAIR, MAP_LINK = 0, 1, 2, 3, 4
OBS_DIM = {OBS_FULL: 33, OBS_IMU: 21}
# the done vector's two element types (QG_DONE_* of include/quadgym.h); the four layers' older names of the pair follow their structs
DONE_U8, DONE_F32 = 0, 1


class QgModel(C.Structure):
    _fields_ = [
        ("timestep", C.c_double),
        ("gravity", C.c_double * 3),
        ("body_parent", C.c_int32 * NBODY),
        ("body_pos", (C.c_double * 3) * NBODY),
        ("body_quat", (C.c_double * 4) * NBODY),
        ("body_mass", C.c_double * NBODY),
        ("body_ipos", (C.c_double * 3) * NBODY),
        ("body_inertia", (C.c_double * 6) * NBODY),
        ("jnt_axis", (C.c_double * 3) * NJNT),
        ("jnt_ref", C.c_double * NJNT),
        ("jnt_range", (C.c_double * 2) * NJNT),
        ("jnt_damping", C.c_double * NJNT),
        ("jnt_armature", C.c_double * NJNT),
        ("free_damping", C.c_double),
        ("free_armature", C.c_double),
        ("act_kp", C.c_double * NU),
        ("act_kv", C.c_double * NU),
        ("act_gear", C.c_double * NU),
        ("act_timeconst", C.c_double * NU),
        ("act_ctrlrange", (C.c_double * 2) * NU),
        ("act_forcerange", (C.c_double * 2) * NU),
        ("limit_stiffness", C.c_double),
        ("limit_damping", C.c_double),
        ("limit_ramp", C.c_double),
        ("ncp", C.c_int32 * NBODY),
        ("cp", ((C.c_double * 3) * MAXCP) * NBODY),
        ("contact_stiffness", C.c_double),
        ("contact_damping", C.c_double),
        ("contact_margin", C.c_double),
        ("contact_friction", C.c_double),
        ("contact_ramp", C.c_double),
        ("qpos0", C.c_double * NQ),
    ]


class QgTask(C.Structure):
    _fields_ = [
        ("frame_skip", C.c_int32),
        ("max_time", C.c_double),
        ("use_time_limit", C.c_int32),
        ("use_fall", C.c_int32),
        ("fall_height", C.c_double),
        ("use_flip", C.c_int32),
        ("w_forward", C.c_double),
        ("w_ctrl", C.c_double),
        ("alive_bonus", C.c_double),
        ("obs_mode", C.c_int32),
        ("sensor_lag", C.c_int32),
        ("auto_reset", C.c_int32),
        ("reset_flags", C.c_uint32),
        ("default_ctrl", C.c_double * NU),
        ("reset_joint_jitter", C.c_double),
    ]


class QgDynamicsRange(C.Structure):
    _fields_ = [("lo", C.c_float * NDYN), ("hi", C.c_float * NDYN)]


# external wrenches (QG_NXFRC / QG_XFRC_* of include/quadgym.h): [n, NBODY, NXFRC] f32, world-frame force xyz and torque xyz per body
NXFRC = 6
XFRC_COLUMNS = ("fx", "fy", "fz", "tx", "ty", "tz")


class QgPushParams(C.Structure):
    """``qg_push_params``: the push schedule of wrench mode (env-steps, N)."""
    _fields_ = [("interval", C.c_int32), ("duration", C.c_int32), ("probability", C.c_float), ("force_min", C.c_float),
                ("force_max", C.c_float)]


class QgCommandSampler(C.Structure):
    """``qg_command_sampler``: the options of ``VelocityHeadingControls.sample`` (``control_inputs.py:74-115``)."""
    _fields_ = [
        ("fixed", C.c_uint32),
        ("min_speed", C.c_double),
        ("max_speed", C.c_double),
        ("fixed_heading_angle", C.c_double),
        ("fixed_velocity_angle", C.c_double),
        ("fixed_speed", C.c_double),
    ]

    @classmethod
    def from_options(cls, options=None):
        o = options or {}
        s = cls()
        s.min_speed, s.max_speed = float(o.get("min_speed", 0.0)), float(o.get("max_speed", 1.0))
        for bit, key, field in ((CMD_FIXED_HEADING, "fixed_heading_angle", "fixed_heading_angle"),
                                (CMD_FIXED_VELOCITY_ANGLE, "fixed_velocity_angle", "fixed_velocity_angle"),
                                (CMD_FIXED_SPEED, "fixed_speed", "fixed_speed")):
            if o.get(key) is not None:
                s.fixed |= bit
                setattr(s, field, float(o[key]))
        return s


class QgWalkParams(C.Structure):
    _fields_ = [
        ("settling_time", C.c_double),
        ("joint_centers", C.c_double * NU),
        ("ema_alpha", C.c_double),
        ("min_freq", C.c_double),
        ("control_cost_alpha", C.c_double),
        ("w", C.c_double * 10),
        ("w_diff_ideal", C.c_double),
        ("body_height", C.c_double),
        ("amp_target", C.c_double * NU),
        ("freq_target", C.c_double * NU),
        ("unit_zero", C.c_int32),
    ]


NWALKREWARD = 11


class _Sized(C.Structure):
    """A struct whose first field is its own size: ``make(**fields)`` fills it in."""

    @classmethod
    def make(cls, **fields):
        s = cls(**fields)
        s.struct_size = C.sizeof(cls)
        return s


class QgPolicyDesc(_Sized):
    """``qg_policy_desc``: the shape of a fused MLP policy (``struct_size`` is filled in)."""
    _fields_ = [("struct_size", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("n_hidden", C.c_int32),
                ("hidden", C.c_int32 * 3), ("out_tanh", C.c_int32), ("has_value", C.c_int32)]

    @classmethod
    def make(cls, obs_dim, hidden, act_dim, out_tanh=False, value=True):
        hidden = [int(h) for h in hidden]
        d = super().make()
        d.obs_dim, d.act_dim, d.n_hidden = int(obs_dim), int(act_dim), len(hidden)
        for i, h in enumerate(hidden[:3]):
            d.hidden[i] = h
        d.out_tanh, d.has_value = int(bool(out_tanh)), int(bool(value))
        return d


class QgPpoParams(_Sized):
    """``qg_ppo_params``: the coefficients of one PPO loss call (``struct_size`` is filled in); ``clip_range_vf=None`` is off."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("clip_range", C.c_float), ("clip_range_vf", C.c_float),
                ("ent_coef", C.c_float), ("vf_coef", C.c_float)]

    @classmethod
    def make(cls, clip_range=0.2, clip_range_vf=None, ent_coef=0.0, vf_coef=0.5):
        d = super().make()
        d.clip_range, d.clip_range_vf = float(clip_range), 0.0 if clip_range_vf is None else float(clip_range_vf)
        d.ent_coef, d.vf_coef = float(ent_coef), float(vf_coef)
        return d


class QgPpoBatch(_Sized):
    """``qg_ppo_batch``: device pointers of one minibatch (``struct_size`` is filled in)."""
    _fields_ = [("struct_size", C.c_int32), ("obs_stride", C.c_int32), ("obs", C.c_void_p), ("actions", C.c_void_p),
                ("old_log_prob", C.c_void_p), ("advantages", C.c_void_p), ("old_values", C.c_void_p), ("returns", C.c_void_p)]

    @classmethod
    def make(cls, obs_stride, **ptrs):
        return super().make(obs_stride=int(obs_stride), **ptrs)


DISTILL_LOSSES = {"mse": 0, "kl": 1}      # QG_DISTILL_MSE, QG_DISTILL_KL


class QgDistillParams(_Sized):
    """``qg_distill_params``: the loss (``"mse"`` / ``"kl"`` or its number) and coefficient of one distillation call (``struct_size`` is
    filled in)."""
    _fields_ = [("struct_size", C.c_int32), ("loss", C.c_int32), ("coef", C.c_float), ("reserved", C.c_int32)]

    @classmethod
    def make(cls, loss="mse", coef=1.0):
        d = super().make()
        d.loss, d.coef = int(DISTILL_LOSSES.get(loss, loss)), float(coef)
        return d


class QgDistillBatch(_Sized):
    """``qg_distill_batch``: device pointers of one minibatch of rows and target means (``struct_size`` is filled in)."""
    _fields_ = [("struct_size", C.c_int32), ("obs_stride", C.c_int32), ("obs", C.c_void_p), ("target_mean", C.c_void_p),
                ("target_log_std", C.c_void_p), ("weights", C.c_void_p)]

    @classmethod
    def make(cls, obs_stride, **ptrs):
        return super().make(obs_stride=int(obs_stride), **ptrs)


class QgAdamParams(_Sized):
    """``qg_adam_params``: the constants of one optimiser step (``struct_size`` is filled in); ``max_grad_norm=None`` is off."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("lr", C.c_float), ("beta_one", C.c_float), ("beta_two", C.c_float),
                ("eps", C.c_float), ("max_grad_norm", C.c_float)]

    @classmethod
    def make(cls, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.5):
        d = super().make()
        d.lr, d.beta_one, d.beta_two, d.eps = float(lr), float(betas[0]), float(betas[1]), float(eps)
        d.max_grad_norm = 0.0 if max_grad_norm is None else float(max_grad_norm)
        return d


class QgNormDesc(_Sized):
    """``qg_norm_desc``: a running normaliser's shape and constants (``struct_size`` is filled in)."""
    _fields_ = [("struct_size", C.c_int32), ("obs_dim", C.c_int32), ("n_envs", C.c_int32), ("gamma", C.c_double),
                ("epsilon", C.c_double), ("clip_obs", C.c_double), ("clip_reward", C.c_double), ("norm_obs", C.c_int32),
                ("norm_reward", C.c_int32)]

    @classmethod
    def make(cls, obs_dim, n_envs, gamma=0.99, epsilon=1e-8, clip_obs=10.0, clip_reward=10.0, norm_obs=True, norm_reward=True):
        d = super().make()
        d.obs_dim, d.n_envs = int(obs_dim), int(n_envs)
        d.gamma, d.epsilon, d.clip_obs, d.clip_reward = float(gamma), float(epsilon), float(clip_obs), float(clip_reward)
        d.norm_obs, d.norm_reward = int(bool(norm_obs)), int(bool(norm_reward))
        return d


NORM_DONE_U8, NORM_DONE_F32 = DONE_U8, DONE_F32


class QgRolloutDesc(_Sized):
    """``qg_rollout_desc``: a rollout buffer's shape and constants (``struct_size`` is filled in)."""
    _fields_ = [("struct_size", C.c_int32), ("n_envs", C.c_int32), ("n_steps", C.c_int32), ("obs_dim", C.c_int32),
                ("act_dim", C.c_int32), ("reserved", C.c_int32), ("gamma", C.c_double), ("gae_lambda", C.c_double)]

    @classmethod
    def make(cls, n_envs, n_steps, obs_dim, act_dim, gamma=0.99, gae_lambda=0.95):
        d = super().make()
        d.n_envs, d.n_steps, d.obs_dim, d.act_dim = int(n_envs), int(n_steps), int(obs_dim), int(act_dim)
        d.gamma, d.gae_lambda = float(gamma), float(gae_lambda)
        return d


class QgRolloutStorage(_Sized):
    """``qg_rollout_storage``: the device arrays the caller owns."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("obs", C.c_void_p), ("actions", C.c_void_p),
                ("log_prob", C.c_void_p), ("values", C.c_void_p), ("rewards", C.c_void_p), ("advantages", C.c_void_p),
                ("returns", C.c_void_p), ("dones", C.c_void_p)]


class QgRolloutStep(_Sized):
    """``qg_rollout_step``: the rows of one env-step."""
    _fields_ = [("struct_size", C.c_int32), ("next_obs_stride", C.c_int32), ("reward_stride", C.c_int32), ("done_kind", C.c_int32),
                ("done_stride", C.c_int32), ("episode_reward_stride", C.c_int32), ("next_obs", C.c_void_p), ("actions", C.c_void_p),
                ("log_prob", C.c_void_p), ("value", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("trunc_value", C.c_void_p), ("episode_reward", C.c_void_p)]


class QgRolloutBatch(_Sized):
    """``qg_rollout_batch``: the outputs of a gather, each nullable."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("obs", C.c_void_p), ("actions", C.c_void_p),
                ("old_log_prob", C.c_void_p), ("old_values", C.c_void_p), ("advantages", C.c_void_p), ("returns", C.c_void_p)]


class QgRolloutInfo(C.Structure):
    """``qg_rollout_info``: the cursor and the two error counters."""
    _fields_ = [("pos", C.c_int32), ("reserved", C.c_int32), ("overflow", C.c_int64), ("bad_index", C.c_int64)]


ROLLOUT_DONE_U8, ROLLOUT_DONE_F32 = DONE_U8, DONE_F32


class QgPerturbDesc(_Sized):
    """``qg_perturb_desc``: the shape, the standard deviations and the key of a perturbation layer (``struct_size`` is filled in)."""
    _fields_ = [("struct_size", C.c_int32), ("n_envs", C.c_int32), ("frame_dim", C.c_int32), ("window", C.c_int32),
                ("max_delay", C.c_int32), ("delay_lo", C.c_int32), ("delay_hi", C.c_int32), ("done_row", C.c_int32),
                ("action_std", C.c_float), ("obs_std", C.c_float * 64), ("bias_std", C.c_float * 64), ("reset_action", C.c_float * NU),
                ("reserved", C.c_int32), ("seed", C.c_uint64), ("env_index_base", C.c_uint64)]

    @classmethod
    def make(cls, n_envs, frame_dim, window=1, max_delay=0, delays=(0, 0), action_std=0.0, obs_std=(), bias_std=(), reset_action=None,
             done_row=0, seed=0, env_index_base=0):
        """``obs_std`` / ``bias_std``: up to ``frame_dim`` values, missing columns are 0.  ``reset_action=None``: the default task's
        ``default_ctrl``."""
        d = super().make()
        d.n_envs, d.frame_dim, d.window, d.max_delay = int(n_envs), int(frame_dim), int(window), int(max_delay)
        d.delay_lo, d.delay_hi, d.done_row = int(delays[0]), int(delays[1]), int(done_row)
        d.action_std = float(action_std)
        for name, vals in (("obs_std", obs_std), ("bias_std", bias_std)):
            vals = [float(v) for v in vals]
            if len(vals) > 64:
                raise ValueError(f"{name}: at most 64 columns, got {len(vals)}")
            for c, v in enumerate(vals):
                getattr(d, name)[c] = v
        if reset_action is None:
            reset_action = (0.0, 0.0, -0.5) * 4             # qg_default_task's default_ctrl (quadruped.py:124)
        if len(reset_action) != NU:
            raise ValueError(f"reset_action: {NU} values, got {len(reset_action)}")
        for j, v in enumerate(reset_action):
            d.reset_action[j] = float(v)
        d.seed, d.env_index_base = int(seed) % (1 << 64), int(env_index_base)
        return d


PERTURB_DONE_ROW_RESET, PERTURB_DONE_ROW_TERMINAL = 0, 1
PERTURB_DONE_U8, PERTURB_DONE_F32 = DONE_U8, DONE_F32
PERTURB_MAX_DELAY = 16


class QgContactDesc(_Sized):
    """``qg_contact_desc``: a contact sensor's constants (``struct_size`` is filled in)."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("force_threshold", C.c_float)]

    @classmethod
    def make(cls, force_threshold=0.0):
        d = super().make()
        d.force_threshold = float(force_threshold)
        return d


CONTACT_DONE_U8, CONTACT_DONE_F32 = DONE_U8, DONE_F32
NFOOT, FOOT_DIM = 4, 12
# the columns of a foot's row (QG_FOOT_* of include/quadgym.h)
FOOT_COLUMNS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "contact", "touchdown", "liftoff", "phase_time", "last_air_time",
                "last_stance_time")
FOOT_BODIES = (3, 6, 9, 12)
MONITOR_MAX_TERMS = 32          # QG_MONITOR_MAX_TERMS
# the gait-shaped reward terms in the order of their columns (QG_GAIT_* of include/quadgym.h)
GAIT_TERMS = ("feet_air_time", "feet_slip", "feet_clearance", "touchdown_speed", "feet_contact_force", "body_contact", "flight")
GAIT_MAX_BASE_TERMS = MONITOR_MAX_TERMS - len(GAIT_TERMS)


class QgGaitDesc(_Sized):
    """``qg_gait_desc``: the weights and thresholds of a gait reward (``struct_size`` is filled in)."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("weights", C.c_float * len(GAIT_TERMS)),
                ("air_time_target", C.c_float), ("clearance_target", C.c_float), ("max_contact_force", C.c_float),
                ("min_command_speed", C.c_float)]

    @classmethod
    def make(cls, weights=(0.0,) * len(GAIT_TERMS), air_time_target=0.0, clearance_target=0.0, max_contact_force=0.0,
             min_command_speed=0.0):
        d = super().make()
        for k, w in enumerate(weights):
            d.weights[k] = float(w)
        d.air_time_target, d.clearance_target = float(air_time_target), float(clearance_target)
        d.max_contact_force, d.min_command_speed = float(max_contact_force), float(min_command_speed)
        return d


# the privileged state pack (qg_priv_*): ``qg_priv_desc`` has the fields of ``qg_contact_desc`` and shares its mirror, ``QgContactDesc``;
# the privileged columns as (name, first column, width) in column order (QG_PRIV_* of include/quadgym.h)
PRIV_COLUMNS = (("base_lin_vel", 0, 3), ("base_ang_vel", 3, 3), ("gravity_dir", 6, 3), ("base_height", 9, 1), ("joint_pos", 10, 12),
                ("joint_vel", 22, 12), ("act", 34, 12), ("foot_contact", 46, 4), ("foot_force", 50, 12), ("foot_height", 62, 4),
                ("body_contact", 66, 1), ("dynamics", 67, NDYN), ("frame_wrench", 78, 6), ("episode_time", 84, 1))
PRIV_DIM = 85

# the commanded gait schedule (qg_sched_*): its reward terms in the order of their columns (QG_SCHED_* of include/quadgym.h), the clock
# columns behind an observation as (name, first column, width), and the limits of its description
SCHED_TERMS = ("swing_force", "stance_velocity", "swing_height", "contact_match")
SCHED_MAX_BASE_TERMS = MONITOR_MAX_TERMS - len(SCHED_TERMS)
SCHED_COLUMNS = (("clock_sin", 0, 4), ("clock_cos", 4, 4), ("gait_freq", 8, 1), ("gait_duty", 9, 1))
SCHED_DIM = 10
SCHED_MAX_GAITS = 8


class QgSchedGait(C.Structure):
    _fields_ = [("offset", C.c_float * 4), ("duty", C.c_float)]


class QgSchedDesc(_Sized):
    """``qg_sched_desc``: the gait table, the draws' ranges and key, the terms' constants and weights (``struct_size`` is filled in)."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("n_gaits", C.c_int32), ("random_phase", C.c_int32),
                ("done_row", C.c_int32), ("freq_lo", C.c_float), ("freq_hi", C.c_float), ("kappa", C.c_float), ("sigma_force", C.c_float),
                ("sigma_velocity", C.c_float), ("swing_height_target", C.c_float), ("min_command_speed", C.c_float),
                ("weights", C.c_float * len(SCHED_TERMS)), ("gaits", QgSchedGait * SCHED_MAX_GAITS), ("seed", C.c_uint64),
                ("env_index_base", C.c_uint64)]

    @classmethod
    def make(cls, gaits=(((0.0, 0.0, 0.0, 0.0), 0.5),), freq=(1.0, 1.0), weights=(0.0,) * len(SCHED_TERMS), random_phase=False, done_row=0,
             kappa=0.0, sigma_force=1.0, sigma_velocity=1.0, swing_height_target=0.0, min_command_speed=0.0, seed=0, env_index_base=0):
        """``gaits``: up to 8 ``(offsets[4], duty)`` rows."""
        d = super().make()
        if len(gaits) > SCHED_MAX_GAITS:
            raise ValueError(f"gaits: at most {SCHED_MAX_GAITS} rows, got {len(gaits)}")
        d.n_gaits, d.random_phase, d.done_row = len(gaits), 1 if random_phase else 0, int(done_row)
        for g, (offsets, duty) in enumerate(gaits):
            if len(offsets) != 4:
                raise ValueError(f"gaits[{g}]: four offsets, got {len(offsets)}")
            for f, off in enumerate(offsets):
                d.gaits[g].offset[f] = float(off)
            d.gaits[g].duty = float(duty)
        d.freq_lo, d.freq_hi, d.kappa = float(freq[0]), float(freq[1]), float(kappa)
        d.sigma_force, d.sigma_velocity = float(sigma_force), float(sigma_velocity)
        d.swing_height_target, d.min_command_speed = float(swing_height_target), float(min_command_speed)
        for k, w in enumerate(weights):
            d.weights[k] = float(w)
        d.seed, d.env_index_base = int(seed) % (1 << 64), int(env_index_base)
        return d


# the command curriculum (qg_cmdcur_*): the limits of its description (QG_CMDCUR_* of include/quadgym.h)
CMDCUR_MAX_SIDE, CMDCUR_MAX_BINS, CMDCUR_MAX_WEIGHT, CMDCUR_MAX_CRITERIA = 16, 256, 65536, 4


class QgCmdCurCriterion(C.Structure):
    _fields_ = [("column", C.c_int32), ("sense", C.c_int32), ("threshold", C.c_float)]


class QgCmdCurDesc(_Sized):
    """``qg_cmdcur_desc``: the grid, the weights' limits, the segment's length and criteria, the key (``struct_size`` is filled in)."""
    _fields_ = [("struct_size", C.c_int32), ("reserved", C.c_int32), ("n_speed", C.c_int32), ("n_alpha", C.c_int32), ("speed_lo", C.c_float),
                ("speed_hi", C.c_float), ("fixed_heading", C.c_int32), ("heading_angle", C.c_float), ("weight_max", C.c_int32),
                ("delta", C.c_int32), ("resample_steps", C.c_int32), ("min_steps", C.c_int32), ("n_criteria", C.c_int32),
                ("reserved2", C.c_int32), ("criteria", QgCmdCurCriterion * CMDCUR_MAX_CRITERIA),
                ("initial_weights", C.c_int32 * CMDCUR_MAX_BINS), ("seed", C.c_uint64), ("env_index_base", C.c_uint64)]

    @classmethod
    def make(cls, speed=(0.0, 1.0), bins=(1, 1), initial_weights=(1,), weight_max=1, delta=1, resample_steps=0, min_steps=1, criteria=(),
             fixed_heading=None, seed=0, env_index_base=0):
        """``criteria``: up to 4 ``(column, sense, threshold)``; ``fixed_heading``: None (theta is drawn) or the angle in rad."""
        d = super().make()
        if len(initial_weights) > CMDCUR_MAX_BINS:
            raise ValueError(f"initial_weights: at most {CMDCUR_MAX_BINS} bins, got {len(initial_weights)}")
        if len(criteria) > CMDCUR_MAX_CRITERIA:
            raise ValueError(f"criteria: at most {CMDCUR_MAX_CRITERIA}, got {len(criteria)}")
        d.n_speed, d.n_alpha = int(bins[0]), int(bins[1])
        d.speed_lo, d.speed_hi = float(speed[0]), float(speed[1])
        d.fixed_heading, d.heading_angle = (0, 0.0) if fixed_heading is None else (1, float(fixed_heading))
        d.weight_max, d.delta, d.resample_steps, d.min_steps = int(weight_max), int(delta), int(resample_steps), int(min_steps)
        d.n_criteria = len(criteria)
        for k, (column, sense, threshold) in enumerate(criteria):
            d.criteria[k].column, d.criteria[k].sense, d.criteria[k].threshold = int(column), int(sense), float(threshold)
        for b, w in enumerate(initial_weights):
            d.initial_weights[b] = int(w)
        d.seed, d.env_index_base = int(seed) % (1 << 64), int(env_index_base)
        return d


def package_dir() -> str:
    return os.path.dirname(os.path.abspath(__file__))


def library_path() -> str:
    # QUADGYM_LIB selects another build of the same library (A/B timing of kernel variants on one box)
    return os.environ.get("QUADGYM_LIB") or os.path.join(package_dir(), "csrc", "libquadgym.so")


_vp, _i32, _f64, _P = C.c_void_p, C.c_int32, C.c_double, C.POINTER
# Every entry point include/quadgym.h declares, in its order: name -> argtypes, or (argtypes, restype) where the result is not the int
# status.  The one list: load_library() applies it, EXPORTS is its keys.  (A <prefix>_state_bytes comes in both forms: the size as
# the int64 result, or the status as the result and the size through an int64 pointer; _TaskLayer.state_bytes reads which from here.)
PROTOTYPES = {
    # the library, the default robot and task
    "qg_version": ([], C.c_char_p),
    "qg_build_id": ([], C.c_char_p),
    "qg_last_error": ([], C.c_char_p),
    "qg_device_pci_bus_id": [_i32, C.c_char_p, _i32],
    "qg_recommended_batch": ([_i32, _i32], _i32),
    "qg_default_model": [_P(QgModel)],
    "qg_default_task": [_P(QgTask)],
    "qg_time_limit_substeps": ([_f64, _f64], C.c_int64),
    # the simulator handle
    "qg_create": [_i32, _i32, _P(QgModel), _P(QgTask), C.c_uint64, _P(_vp)],
    "qg_destroy": [_vp],
    "qg_num_envs": [_vp],
    "qg_obs_dim": [_vp],
    "qg_reset": [_vp, _vp, C.c_uint64, C.c_uint32],
    "qg_step": [_vp, _vp, _vp, _vp, _vp, _vp],
    "qg_step_device": [_vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "qg_step_device_packed": [_vp, _vp, _vp, _vp],
    "qg_get_state": [_vp, _vp, _vp, _vp, _vp, _vp],
    "qg_step_mirror": [_vp] * 11,
    "qg_set_state": [_vp, _vp, _vp, _vp, _vp, _vp],
    "qg_time_step_kernel": [_vp, _vp, _vp, _i32, _P(C.c_float)],
    "qg_set_track_ctrl": [_vp, _i32],
    "qg_debug_phase_times": [_vp],
    "qg_debug_last_step_kernel": [_vp, C.c_char_p, _i32],
    "qg_set_task": [_vp, _P(QgTask)],
    "qg_get_task": [_vp, _P(QgTask)],
    "qg_uses_baked_model": [_vp],
    "qg_set_mapping": [_vp, _i32],
    "qg_get_mapping": [_vp],
    # the per-step exchange between GPUs
    "qg_comm_unique_id": [_vp],
    "qg_comm_create": [_vp, _i32, _i32, _vp, _P(_vp)],
    "qg_comm_destroy": [_vp],
    "qg_comm_rollout": [_vp, _vp, _i32, _vp, _vp, _i32, _i32],
    "qg_comm_synchronize": [_vp],
    # the walking task and the partially observable pack
    "qg_walk_default_params": [_P(QgWalkParams)],
    "qg_walk_create": [_vp, _P(QgWalkParams), _P(_vp)],
    "qg_walk_destroy": [_vp],
    "qg_walk_set_commands": [_vp, _vp, _vp],
    "qg_walk_reset": [_vp, _vp, C.c_uint64, C.c_uint32],
    "qg_walk_step": [_vp, _vp, _vp, _vp, _vp, _vp],
    "qg_walk_step_device": [_vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "qg_walk_get_estimates": [_vp, _vp, _vp, _vp],
    "qg_walk_set_command_sampler": [_vp, _vp],
    "qg_walk_get_commands": [_vp, _vp, _vp],
    "qg_po_create": [_vp, _i32, _P(_vp)],
    "qg_po_destroy": [_vp],
    "qg_po_obs_dim": [_vp],
    "qg_po_reset": [_vp, _vp, C.c_uint64, C.c_uint32, _vp],
    "qg_po_step": [_vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "qg_po_step_device": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    # snapshots of the task layers and the reset streams
    "qg_walk_state_bytes": ([_vp], C.c_int64),
    "qg_walk_get_state": [_vp, _vp],
    "qg_walk_set_state": [_vp, _vp],
    "qg_po_state_bytes": ([_vp], C.c_int64),
    "qg_po_get_state": [_vp, _vp],
    "qg_po_set_state": [_vp, _vp],
    "qg_get_reset_streams": [_vp, _vp, _P(C.c_uint64)],
    "qg_set_reset_streams": [_vp, _vp, C.c_uint64],
    # many env-steps per launch; the resident mode
    "qg_step_device_seq": [_vp, _vp, _vp, _i32, _vp],
    "qg_resident_start": [_vp, _i32, _i32, _vp, _vp],
    "qg_resident_stop": [_vp],
    "qg_resident_buffers": [_vp, _P(_vp), _P(_vp), _P(_i32)],
    "qg_resident_step_device": [_vp, _i32, _vp],
    "qg_resident_ensure": [_vp],
    "qg_resident_status": [_vp, _P(C.c_int64), _P(_i32), _P(C.c_int64), _P(C.c_int64)],
    # per-env dynamics, external wrenches, pushes
    "qg_set_dynamics_range": [_vp, _P(QgDynamicsRange)],
    "qg_set_dynamics": [_vp, _vp, _vp],
    "qg_get_dynamics": [_vp, _vp],
    "qg_clear_dynamics": [_vp],
    "qg_set_xfrc": [_vp, _vp, _vp],
    "qg_set_xfrc_device": [_vp, _vp, _vp],
    "qg_get_xfrc": [_vp, _vp],
    "qg_set_push": [_vp, _P(QgPushParams)],
    "qg_clear_xfrc": [_vp],
    # the fused MLP policy: forward, PPO gradient, Adam
    "qg_policy_create": [_i32, _P(QgPolicyDesc), _P(_vp)],
    "qg_policy_destroy": [_vp],
    "qg_policy_param_count": [_P(QgPolicyDesc)],
    "qg_policy_set_params": [_vp, _vp],
    "qg_policy_get_params": [_vp, _vp],
    "qg_policy_set_params_device": [_vp, _vp, _vp],
    "qg_policy_forward_device": [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp],
    "qg_policy_launch_shape": [_vp, _i32, _i32, _P(_i32), _P(_i32)],
    "qg_policy_create_asym": [_i32, _P(QgPolicyDesc), _i32, _i32, _P(_vp)],
    "qg_policy_param_count_asym": [_P(QgPolicyDesc), _i32],
    "qg_policy_critic_window": [_vp, _P(_i32), _P(_i32)],
    "qg_policy_reserve_grad": [_vp, _i32],
    "qg_policy_ppo_grad_device": [_vp, _P(QgPpoParams), _i32, _P(QgPpoBatch), _vp, _vp, _vp],
    "qg_policy_distill_grad_device": [_vp, _vp, _i32, _vp, _vp, _vp, _vp],      # (params and batch: byref of policy.py's mirrors)
    "qg_policy_reserve_adam": [_vp],
    "qg_policy_adam_update_device": [_vp, _P(QgAdamParams), _vp, _vp, _vp, _vp, _vp],
    "qg_policy_adam_get_state": [_vp, _vp, _vp, _P(C.c_int64)],
    "qg_policy_adam_set_state": [_vp, _vp, _vp, C.c_int64],
    "qg_policy_normalize_advantages_device": [_vp, _i32, _vp, _vp, _vp],
    # running normalisation
    "qg_norm_create": [_i32, _P(QgNormDesc), _P(_vp)],
    "qg_norm_destroy": [_vp],
    "qg_norm_step_device": [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp],
    "qg_norm_update_obs_device": [_vp, _i32, _vp, _i32, _vp],
    "qg_norm_apply_obs_device": [_vp, _i32, _vp, _i32, _vp, _i32, _vp],
    "qg_norm_reset_returns_device": [_vp, _vp],
    "qg_norm_get_state": [_vp] * 8,
    "qg_norm_set_state": [_vp, _vp, _vp, _f64, _f64, _f64, _f64, _vp],
    # the rollout buffer
    "qg_rollout_create": [_i32, _P(QgRolloutDesc), _P(QgRolloutStorage), _P(_vp)],
    "qg_rollout_destroy": [_vp],
    "qg_rollout_begin_device": [_vp, _vp, _i32, _vp],
    "qg_rollout_add_device": [_vp, _P(QgRolloutStep), _vp],
    "qg_rollout_compute_device": [_vp, _vp, _vp],
    "qg_rollout_gather_device": [_vp, _vp, _i32, _P(QgRolloutBatch), _vp],
    "qg_rollout_get_info": [_vp, _P(QgRolloutInfo)],
    "qg_rollout_episode_stats": [_vp, _P(_f64), _P(C.c_int64), _P(C.c_int64), _i32],
    # sensor noise, bias and actuation latency
    "qg_perturb_create": [_i32, _P(QgPerturbDesc), _P(_vp)],
    "qg_perturb_destroy": [_vp],
    "qg_perturb_actions_device": [_vp, _i32, _vp, _vp, _vp],
    "qg_perturb_observe_device": [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp],
    "qg_perturb_begin_device": [_vp, _i32, _vp, _vp, _i32, _vp],
    "qg_perturb_get_delays": [_vp, _vp],
    "qg_perturb_get_state": [_vp, _vp, _vp, _vp],
    "qg_perturb_set_state": [_vp, _vp, _vp, _vp],
    # the contact sensor
    "qg_contact_create": [_vp, _P(QgContactDesc), _P(_vp)],
    "qg_contact_destroy": [_vp],
    "qg_contact_reset": [_vp, _vp],
    "qg_contact_read_device": [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "qg_contact_read": [_vp, _vp, _vp],
    "qg_contact_state_bytes": ([_vp], C.c_int64),
    "qg_contact_get_state": [_vp, _vp],
    "qg_contact_set_state": [_vp, _vp],
    # the reward monitor
    "qg_monitor_create": [_i32, _i32, _i32, _i32, _P(_vp)],
    "qg_monitor_destroy": [_vp],
    "qg_monitor_record_device": [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp],
    "qg_monitor_reset": [_vp, _vp, _i32, _i32],
    "qg_monitor_get_info": [_vp, _P(C.c_int64), _P(C.c_int64), _P(C.c_int64), _vp, _i32],
    "qg_monitor_get_state": [_vp, _vp, _vp, _vp, _P(C.c_int64), _P(C.c_int64), _P(C.c_int64)],
    "qg_monitor_set_state": [_vp, _vp, _vp, _vp, C.c_int64, C.c_int64, C.c_int64],
    # the gait-shaped reward terms
    "qg_gait_create": [_vp, _P(QgGaitDesc), _P(_vp)],
    "qg_gait_destroy": [_vp],
    "qg_gait_set_weights": [_vp, _P(C.c_float)],
    "qg_gait_reward_device": [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp],
    # the privileged state pack
    "qg_priv_create": [_vp, _P(QgContactDesc), _P(_vp)],       # (qg_priv_desc: the layout of qg_contact_desc)
    "qg_priv_destroy": [_vp],
    "qg_priv_read_device": [_vp, _vp, _i32, _i32, _vp, _i32, _vp],
    "qg_priv_read": [_vp, _vp],
    # the commanded gait schedule
    "qg_sched_create": [_vp, _P(QgSchedDesc), _P(_vp)],
    "qg_sched_destroy": [_vp],
    "qg_sched_set_weights": [_vp, _P(C.c_float)],
    "qg_sched_advance_device": [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _i32,
                             _vp, _i32, _vp, _i32, _vp],
    "qg_sched_begin_device": [_vp, _vp, _vp, _i32, _i32, _vp],
    "qg_sched_get_gaits": [_vp, _vp, _vp, _vp],
    "qg_sched_state_bytes": [_vp, _P(C.c_int64)],
    "qg_sched_get_state": [_vp, _vp],
    "qg_sched_set_state": [_vp, _vp],
    # the command curriculum
    "qg_cmdcur_create": [_vp, _P(QgCmdCurDesc), _P(_vp)],
    "qg_cmdcur_destroy": [_vp],
    "qg_cmdcur_advance_device": [_vp, _vp, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _vp],
    "qg_cmdcur_begin_device": [_vp, _vp, _vp],
    "qg_cmdcur_get_weights": [_vp, _vp],
    "qg_cmdcur_set_weights": [_vp, _vp],
    "qg_cmdcur_get_stats": [_vp, _vp, _vp],
    "qg_cmdcur_get_bins": [_vp, _vp, _vp, _vp],
    "qg_cmdcur_state_bytes": [_vp, _P(C.c_int64)],
    "qg_cmdcur_get_state": [_vp, _vp],
    "qg_cmdcur_set_state": [_vp, _vp],
}
EXPORTS = tuple(PROTOTYPES)


_lib = None


def load_library():
    """Load ``libquadgym.so`` and declare the prototypes of every exported entry
    point (``include/quadgym.h``).  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C quadruped-gym_amd/csrc`). "
            "There is no CPU fallback.")
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 (same SONAME as the system's).  Loaded after
    # ours it becomes a SECOND runtime and torch then finds no GPU; loaded first, libquadgym.so's dependency resolves
    # to that same copy.  So when torch is installed, load it before the library.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(path)
    for name, proto in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = proto if isinstance(proto, tuple) else (proto, C.c_int)
    _lib = lib
    return lib


class QuadGymError(RuntimeError):
    pass


def check(status: int, what: str):
    if status != 0:
        msg = load_library().qg_last_error().decode("utf-8", "replace")
        raise QuadGymError(f"{what} failed ({status}): {msg}")


def recommended_batch(n_envs: int, device: int = -1) -> int:
    """The batch size at the top of the step-time stair ``n_envs`` stands on (``qg_recommended_batch``): 4096, 16 384, then multiples
    of 32 768 on an MI355X.  ``device=-1`` assumes an MI355X (no GPU needed)."""
    return int(load_library().qg_recommended_batch(int(n_envs), int(device)))


def push_params(spec: dict | None) -> QgPushParams | None:
    """``qg_push_params`` from ``{"interval": env-steps, "duration": env-steps, "probability": p, "force": (lo, hi) N}``; None: no
    schedule."""
    if spec is None:
        return None
    unknown = set(spec) - {"interval", "duration", "probability", "force"}
    if unknown:
        raise ValueError(f"push schedule keys {sorted(unknown)}: one of interval, duration, probability, force")
    lo, hi = spec["force"]
    return QgPushParams(int(spec["interval"]), int(spec["duration"]), float(spec["probability"]), float(lo), float(hi))


def push_schedule_steps(spec: dict, step_seconds: float) -> dict:
    """The VecEnvs' ``push_randomization={"interval_s", "duration_s", "probability", "force": (lo, hi)}`` as the env-step schedule of
    ``BatchedSim.set_push_schedule``: seconds / (timestep x frame_skip), rounded to nearest, at least 1 env-step."""
    unknown = set(spec) - {"interval_s", "duration_s", "probability", "force"}
    if unknown:
        raise ValueError(f"push_randomization keys {sorted(unknown)}: one of interval_s, duration_s, probability, force")

    def steps(seconds):
        return max(1, int(round(float(seconds) / float(step_seconds))))
    return {"interval": steps(spec["interval_s"]), "duration": steps(spec["duration_s"]), "probability": float(spec["probability"]),
            "force": tuple(float(f) for f in spec["force"])}


def identity_dynamics_row(model: QgModel):
    """The row that leaves ``model`` as it is: ``(contact_friction, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1)`` (f32)."""
    import numpy as np
    row = np.ones(NDYN, np.float32)
    row[0] = np.float32(model.contact_friction)
    row[1:5] = 0.0
    return row


def dynamics_range(spec: dict, model: QgModel) -> QgDynamicsRange:
    """``qg_dynamics_range`` from a dict: ``{"friction": (lo, hi), "payload_mass": (lo, hi), "payload_pos": ((lo, hi), (lo, hi),
    (lo, hi)), "kp_scale": (lo, hi), ...}`` -- the column names of ``DYN_COLUMNS`` (``payload_pos`` for x, y, z).  Missing keys stay at
    the identity."""
    ident = identity_dynamics_row(model)
    lo, hi = ident.copy(), ident.copy()
    for key, val in spec.items():
        if key == "payload_pos":
            pairs = list(val)
            if len(pairs) != 3:
                raise ValueError("payload_pos: three (lo, hi) pairs, for x, y and z")
            for d, pair in enumerate(pairs):
                lo[2 + d], hi[2 + d] = pair
        elif key in DYN_COLUMNS and key not in ("payload_x", "payload_y", "payload_z"):
            lo[DYN_COLUMNS.index(key)], hi[DYN_COLUMNS.index(key)] = val
        else:
            raise ValueError(f"dynamics key {key!r}: one of friction, payload_mass, payload_pos, " + ", ".join(DYN_COLUMNS[5:]))
    r = QgDynamicsRange()
    for c in range(NDYN):
        r.lo[c], r.hi[c] = float(lo[c]), float(hi[c])
    return r


def default_model() -> QgModel:
    m = QgModel()
    check(load_library().qg_default_model(C.byref(m)), "qg_default_model")
    return m


def default_task() -> QgTask:
    t = QgTask()
    check(load_library().qg_default_task(C.byref(t)), "qg_default_task")
    return t
