"""The definition of the gait-shaped reward terms (include/quadgym.h, "gait-shaped reward terms from the foot-contact sensor") in NumPy,
as a function of what the launch reports and takes -- (body_force, feet, done, command, reward, base) plus the parameters --, evaluated
in float64 or in float32 in the stated order; the term names, the parameters, walk recipe and synthetic rows the CPU and GPU tests
share, and the error budget measured by tests/test_gait_reward_reference.py.  No GPU, no torch."""
import numpy as np

import shaped_reward_reference as S

TERMS = ("feet_air_time", "feet_slip", "feet_clearance", "touchdown_speed", "feet_contact_force", "body_contact", "flight")
NTERMS = len(TERMS)
FEET = (3, 6, 9, 12)
NON_FEET = tuple(b for b in range(13) if b not in FEET)
# the QG_FOOT_* columns
POS_Z, VEL_X, VEL_Y, VEL_Z, CONTACT, TOUCHDOWN, LAST_AIR_TIME = 2, 3, 4, 5, 6, 7, 10

# ---- the parameters the tests share ----------------------------------------------------------------------------------------------------
FORCE_THRESHOLD = 1.0
MAX_CONTACT_FORCE = 20.0
CLEARANCE_TARGET = 0.05
MIN_COMMAND_SPEED = 0.1
WEIGHTS = {"feet_air_time": 2.0, "feet_slip": -0.25, "feet_clearance": -30.0, "touchdown_speed": -0.5, "feet_contact_force": -0.01,
           "body_contact": -1.0, "flight": 0.75}                  # all non-zero, mixed signs
# The walk recipe (tests/test_zz_contact_sensor_gpu.py's proven one): 67 envs, 80 env-steps, the default task with auto_reset, a time
# limit of 0.2 s (25 env-steps per episode) and fall / flip off, uniform actions of seed 3, sim.reset(seed=1).
N_WALK, T_WALK, WALK_ACTION_SEED, WALK_RESET_SEED, WALK_MAX_TIME = 67, 80, 3, 1, 0.2
DT = 0.008                                                        # model.timestep x frame_skip
# air_time_target = (k + 0.5) dt: never equal to an air time (whole env-steps x dt).  k was chosen once from the recorded walk run: the
# completed swings at its 1492 touchdowns last 1 .. 24 env-steps, 570 of them at most 2 and 922 more, so feet_air_time takes both signs.
AIR_TIME_K = 2
AIR_TIME_TARGET = (AIR_TIME_K + 0.5) * DT
PARAMS = dict(weights=WEIGHTS, air_time_target=AIR_TIME_TARGET, clearance_target=CLEARANCE_TARGET, max_contact_force=MAX_CONTACT_FORCE,
              min_command_speed=MIN_COMMAND_SPEED)

# ---- the measured error budget (tests/test_gait_reward_reference.py prints a fresh measurement and fails if it exceeds these) ---------
# The largest deviation of the float32 evaluation in the stated order from the float64 evaluation of the same float32 rows, over the 664
# states of tests/golden/contact_cells.npz with synthetic events, per UNWEIGHTED term as (atol, rtol): |t32 - t64| <= atol + rtol |t64|.
# Where the sizes come from.  Every term is a sum of at most four non-negative products of two or three float32 factors: a relative
# error of a few eps (6e-8), no cancellation -- except feet_air_time, a sum of differences (air time - target) of either sign whose
# operands are up to a tenth of a second: an absolute error of half an ulp of those (3.7e-9).  feet_contact_force subtracts the 20 N
# threshold from a larger float32 force: exact or nearly so, what is left is the sum's rounding.  body_contact and flight are small
# integers: exact.
# measured: feet_air_time |err| <= 3.73e-9 s (share of the bound 0.75); relative errors feet_slip 9.5e-8 (0.63), feet_clearance 1.84e-7
# (0.61), touchdown_speed 5.8e-8 (0.58), feet_contact_force 2.4e-8 (0.47)
BUDGET_TERM = {
    "feet_air_time": (5.0e-9, 0.0),
    "feet_slip": (0.0, 1.5e-7),
    "feet_clearance": (0.0, 3.0e-7),
    "touchdown_speed": (0.0, 1.0e-7),
    "feet_contact_force": (0.0, 5.0e-8),
    "body_contact": (0.0, 0.0),
    "flight": (0.0, 0.0),
}
# the float32 sum of the seven components and the add onto the reward: 7 roundings of at most half an ulp of the running magnitude
BUDGET_SUM_ULPS = 7
MARGIN = 4.0          # a different but equally valid rounding order (contraction into fma, sqrt), as tests/contact_sensor_reference.py


def weight_vector(weights, dtype=np.float64):
    """[7] in the order of TERMS, as the float32 values the C ABI takes."""
    return S.weight_vector(weights, TERMS, dtype)


def evaluate(body_force, feet, done=None, command=None, reward=None, base=None, *, weights, air_time_target, clearance_target,
             max_contact_force, min_command_speed, force_threshold, dtype=np.float64):
    """The definition on rows as the launch reports them: body_force [n, 13, 3], feet [n, 4, 12] (float32); done [n] or None;
    command [n, 2] or None; reward [n] or None; base [n, C0] or None.  The parameters enter as the float32 values the C ABI takes; every
    operation then runs in `dtype`, sums in ascending order.  Returns a dict: terms [n, 7] (unweighted, the gate applied, finished envs
    NOT zeroed), components [n, 7], shaped [n], reward_out [n], wide [n, C0 + 7]."""
    T = dtype
    f32 = lambda v: np.float32(v).astype(T)
    force, rows = np.asarray(body_force, np.float32), np.asarray(feet, np.float32)
    n = len(rows)
    r = rows.astype(T)
    c, td = r[..., CONTACT], r[..., TOUCHDOWN]
    planar = r[..., VEL_X] * r[..., VEL_X] + r[..., VEL_Y] * r[..., VEL_Y]
    lift = r[..., POS_Z] - f32(clearance_target)
    fz = force[..., 2]
    per_foot = [td * (r[..., LAST_AIR_TIME] - f32(air_time_target)),
                c * planar,
                (T(1) - c) * (lift * lift * np.sqrt(planar)),
                td * (r[..., VEL_Z] * r[..., VEL_Z]),
                np.maximum(fz[:, list(FEET)].astype(T) - f32(max_contact_force), T(0))]
    terms = np.zeros((n, NTERMS), T)
    for k, a in enumerate(per_foot):
        s = a[:, 0].astype(T)
        for f in range(1, 4):                                     # ascending f
            s = (s + a[:, f]).astype(T)
        terms[:, k] = s
    terms[:, 5] = (fz[:, list(NON_FEET)] > np.float32(force_threshold)).sum(1)         # exact f32 comparison
    terms[:, 6] = (rows[..., CONTACT].sum(1) == 0)
    if command is not None:
        cmd = np.asarray(command, np.float32)
        gate = np.maximum(np.abs(cmd[:, 0]), np.abs(cmd[:, 1])) > np.float32(min_command_speed)
        terms[:, 0] = np.where(gate, terms[:, 0], T(0))
    return dict(S.tail(terms, weights, TERMS, done, reward, base, T), terms=terms)


def term_tolerance(terms64, margin=1.0):
    """[n, 7]: margin x (atol + rtol |t64|) per unweighted term."""
    return S.term_tolerance(terms64, TERMS, BUDGET_TERM, margin)


def component_tolerance(ref, weights, margin=1.0):
    """[n, 7]: the terms' bounds times |w_k|, and the one rounding of f32(w_k x term_k)."""
    return S.component_tolerance(ref, weights, TERMS, BUDGET_TERM, margin)


def reward_tolerance(ref, weights, reward=None, margin=1.0):
    """[n]: the components' bounds summed, and BUDGET_SUM_ULPS roundings of half an ulp of the magnitudes added."""
    return S.reward_tolerance(ref, weights, TERMS, BUDGET_TERM, BUDGET_SUM_ULPS, reward, margin)


# ---- synthetic rows on the fixture's states ----------------------------------------------------------------------------------------------
def fixture_rows(sensor_ref, seed=11):
    """(body_force [664, 13, 3], feet [664, 4, 12]) float32 from tests/contact_sensor_reference.evaluate's result on the fixture: the
    contact flag at FORCE_THRESHOLD, and synthetic events -- half of the feet in contact touch down in this sample, after a swing of
    1 .. 12 env-steps."""
    rng = np.random.default_rng(seed)
    force = sensor_ref["force"].astype(np.float32)
    contact = force[:, list(FEET), 2] > np.float32(FORCE_THRESHOLD)
    n = len(force)
    touchdown = contact & (rng.random((n, 4)) < 0.5)
    air_steps = rng.integers(1, 13, (n, 4))
    feet = np.zeros((n, 4, 12), np.float32)
    feet[..., 0:3], feet[..., 3:6] = sensor_ref["foot_pos"], sensor_ref["foot_vel"]
    feet[..., CONTACT], feet[..., TOUCHDOWN] = contact, touchdown
    feet[..., 9] = np.float32(1) * np.float32(DT)
    feet[..., LAST_AIR_TIME] = air_steps.astype(np.float32) * np.float32(DT)
    return force, feet


def fixture_extras(n, seed=12):
    """(done [n] bool, command [n, 2] f32, reward [n] f32, base [n, 11] f32): every tenth env finished; commands on both sides of
    MIN_COMMAND_SPEED and some exactly on it."""
    rng = np.random.default_rng(seed)
    done = np.arange(n) % 10 == 7
    command = rng.uniform(-0.3, 0.3, (n, 2)).astype(np.float32)
    command[::9] = (np.float32(MIN_COMMAND_SPEED), np.float32(-0.05))
    reward = rng.normal(0.0, 2.0, n).astype(np.float32)
    base = rng.normal(0.0, 1.0, (n, 11)).astype(np.float32)
    return done, command, reward, base


# ---- the walk recipe --------------------------------------------------------------------------------------------------------------------
def walk_task(abi):
    t = abi.default_task()
    t.auto_reset, t.use_time_limit, t.max_time, t.use_fall, t.use_flip = 1, 1, WALK_MAX_TIME, 0, 0
    return t


def walk_actions():
    """[T_WALK, N_WALK, 12] float32."""
    return np.random.default_rng(WALK_ACTION_SEED).uniform(-1, 1, (T_WALK, N_WALK, 12)).astype(np.float32)
