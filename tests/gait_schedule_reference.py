"""The definition of the commanded gait schedule (include/quadgym.h, "commanded gait schedule") in NumPy: the phase, the table integers
and the draws in exact integers -- k(s) is tests/perturb_reference.py's, in the schedule's key space --, the foot quantities, terms and
clock columns in float64 or in float32 in the stated order; the parameters, scripted done table and fixture states the CPU and GPU
tests share, and the error budget measured by tests/test_gait_schedule_reference.py.  No GPU, no torch."""
import numpy as np

import perturb_reference as P
import shaped_reward_reference as S

TERMS = ("swing_force", "stance_velocity", "swing_height", "contact_match")
NTERMS, DIM = len(TERMS), 10
FEET = (3, 6, 9, 12)
SALT = 0x5147534348454431                                         # "QGSCHED1"
M32 = np.uint64(0xFFFFFFFF)
POS_Z, VEL = 2, slice(3, 6)                                       # the QG_FOOT_* columns read here

# ---- the parameters the tests share ----------------------------------------------------------------------------------------------------
# the presets written out for quadruped.xml's legs 1..4 at (-x, +y), (-x, -y), (+x, -y), (+x, +y): (offsets, duty)
GAITS = {"trot": ((0.0, 0.5, 0.0, 0.5), 0.5), "pace": ((0.0, 0.5, 0.5, 0.0), 0.5), "bound": ((0.0, 0.0, 0.5, 0.5), 0.5),
         "pronk": ((0.0, 0.0, 0.0, 0.0), 0.5), "walk": ((0.0, 0.5, 0.75, 0.25), 0.75)}
TABLE = tuple(GAITS[name] for name in ("trot", "pace", "bound", "pronk", "walk"))
FREQ = (1.0, 3.0)                                                 # Hz: at 3 Hz the phase wraps 2.4 times in STEPS env-steps
TIMESTEP, FRAME_SKIP, STEPS = 0.002, 10, 40                       # dt = 0.02 s
DT32 = np.float32(np.float64(TIMESTEP) * FRAME_SKIP)
SEEDS = (0, 1, 12345)
FORCE_THRESHOLD = 1.0
KAPPA = 1.0 / 256
WEIGHTS = {"swing_force": -0.5, "stance_velocity": -0.25, "swing_height": -30.0, "contact_match": 0.125}      # all non-zero, mixed signs
LIMITS = dict(kappa=KAPPA, sigma_force=5.0, sigma_velocity=0.5, swing_height_target=0.05, min_command_speed=0.1)
PARAMS = dict(LIMITS, gaits=TABLE, freq=FREQ, weights=WEIGHTS, random_phase=True)
SIZES = (1, 5, 67)                                                # 67: no multiple of the 4 envs of a wave, nor of 64
C0 = 11

# ---- the measured error budget (tests/test_gait_schedule_reference.py prints a fresh measurement and fails if it exceeds these) ------
# The largest deviation of the float32 evaluation in the stated order from the float64 evaluation of the same float32 rows and the same
# integers, over the 67 fixture states x STEPS phases x SEEDS, per UNWEIGHTED term as (atol, rtol): |t32 - t64| <= atol + rtol |t64|.
# Where the sizes come from.  s_f, p_f and d are exact in float32 (the ramp's product m * inv2k is a float32 times a power of two here).
# swing_force and stance_velocity are sums of at most four products (1 - s)(1 - exp(-x)) in [0, 1]: exp's argument carries three
# roundings of x (relative 2e-7, so absolute 2e-7 x exp(-x) <= 7e-8 in the value) and 1 - exp(-x) one more of half an ulp of 1 -- an
# absolute error of up to 1e-7 per foot.  The forces are tens of sigma_force^2 where a foot stands (exp underflows to 0: exact) and 0
# where it does not, so swing_force sees little of it; the feet's speeds are of the order of sigma_velocity, so stance_velocity sees
# all of it in each of four feet.  swing_height is a sum of four products of float32 factors: relative, a few eps.  contact_match is a
# small integer: exact.
# measured: swing_force |err| <= 7.9e-8 (share 0.66), stance_velocity 2.57e-7 (0.73), swing_height relative 1.74e-7 (0.70)
BUDGET_TERM = {
    "swing_force": (1.2e-7, 0.0),
    "stance_velocity": (3.5e-7, 0.0),
    "swing_height": (0.0, 2.5e-7),
    "contact_match": (0.0, 0.0),
}
# the clock's sin / cos columns, budgeted as tests/perturb_reference.py budgets z's cospif: E_clock is the largest deviation of the
# float32 NumPy evaluation sin(f32(2 pi) * p) / cos(...) from the float64 one over the same phases.  f32(2 pi) is off by 1.7e-7
# (relative 2.8e-8) and the product rounds once more: up to 6.28 x (2.8e-8 + 6e-8) = 5.5e-7 in the argument, and as much in the value.
# measured: 4.10e-7 (share 0.68)
BUDGET_CLOCK = 6.0e-7
BUDGET_SUM_ULPS = 4   # the float32 sum of the four components and the add onto the reward: roundings of half an ulp of the running magnitude
MARGIN = 4.0          # a different but equally valid rounding order, as tests/gait_reward_reference.py and tests/contact_sensor_reference.py


# ---- exact integers -----------------------------------------------------------------------------------------------------------------------
def k(seed, env, episode, stream):
    """k(s) of the schedule's key space: perturb_reference's hash with seed + SALT."""
    return P.k_int(int(seed) + SALT, env, episode, stream, salted=False)


def table_ints(gaits=TABLE):
    """(off [G, 4], D [G]) uint64 (< 2^32): off_f = rint(f64(f32 offset) * 2^32) mod 2^32, D = rint(f64(f32 duty) * 2^32)."""
    off = [[int(np.rint(np.float64(np.float32(o)) * 2.0 ** 32)) % (1 << 32) for o in offsets] for offsets, _ in gaits]
    D = [int(np.rint(np.float64(np.float32(duty)) * 2.0 ** 32)) for _, duty in gaits]
    return np.array(off, np.uint64), np.array(D, np.uint64)


def draws(seed, env, episode, n_gaits=len(TABLE), freq=FREQ, random_phase=True):
    """(g int64, freq float32, phi0 uint64) of the episodes `episode` of the envs `env` (arrays)."""
    f32 = np.float32
    env, episode = np.asarray(env, np.int64), np.asarray(episode, np.int64)
    g = (k(seed, env, episode, 0) * n_gaits) >> 24
    lo, span = f32(freq[0]), f32(f32(freq[1]) - f32(freq[0]))
    u = k(seed, env, episode, 1).astype(f32) * f32(2.0 ** -24)
    fr = (lo + (span * u).astype(f32)).astype(f32)
    phi0 = (k(seed, env, episode, 2).astype(np.uint64) << np.uint64(8)) if random_phase else np.zeros(len(g), np.uint64)
    return g, fr, phi0


def dphi(freq, dt32=DT32):
    return np.rint(np.asarray(freq, np.float32).astype(np.float64) * np.float64(np.float32(dt32)) * 2.0 ** 32).astype(np.uint64)


class Checker:
    """The oscillators of n envs in exact integers.  `step(done)` returns the two views the launch writes columns for -- (phi, g,
    freq) of the row and of the old episode after its advance -- and moves the state on."""

    def __init__(self, n, gaits=TABLE, freq=FREQ, random_phase=True, done_row="terminal", seed=0, env_index_base=0, dt32=DT32, **_):
        self.n, self.n_gaits, self.freq, self.random_phase = n, len(gaits), freq, random_phase
        self.done_row, self.seed, self.dt32 = done_row, seed, dt32
        self.env = env_index_base + np.arange(n, dtype=np.int64)
        self.episode = np.zeros(n, np.int64)
        self.phi = self.draw(self.episode)[2]

    def draw(self, episode):
        return draws(self.seed, self.env, episode, self.n_gaits, self.freq, self.random_phase)

    def gaits(self):
        g, fr, _ = self.draw(self.episode)
        return dict(gait=g, freq=fr, phi=self.phi.copy())

    def step(self, done=None):
        fin = np.zeros(self.n, bool) if done is None else np.asarray(done) != 0
        g, fr, _ = self.draw(self.episode)
        adv = (self.phi + dphi(fr, self.dt32)) & M32
        g1, fr1, phi1 = self.draw(self.episode + 1)
        old = dict(phi=adv, g=g, freq=fr)
        reset = fin & (self.done_row == "reset")
        row = dict(phi=np.where(reset, phi1, adv), g=np.where(reset, g1, g), freq=np.where(reset, fr1, fr))
        self.episode = self.episode + fin
        self.phi = np.where(fin, phi1, adv)
        return row, old

    def begin(self, mask=None):
        sel = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        self.episode = self.episode + sel
        g, fr, phi0 = self.draw(self.episode)
        self.phi = np.where(sel, phi0, self.phi)
        return dict(phi=self.phi.copy(), g=g, freq=fr), sel


# ---- floats ---------------------------------------------------------------------------------------------------------------------------------
def foot_quantities(phi, g, gaits=TABLE, kappa=KAPPA, dtype=np.float64):
    """(hard [n, 4] bool, p [n, 4], d [n], s [n, 4]) of the phases `phi` under the gait rows `g`; p, d, s in `dtype`."""
    T = dtype
    off, D = table_ints(gaits)
    q = (np.asarray(phi, np.uint64)[:, None] + off[g]) & M32
    Dg = D[g]
    hard = q < Dg[:, None]
    p = (q >> np.uint64(8)).astype(T) * T(2.0 ** -24)
    d = (Dg >> np.uint64(8)).astype(T) * T(2.0 ** -24)
    m = np.where(hard, np.minimum(p, d[:, None] - p), -np.minimum(p - d[:, None], T(1) - p)).astype(T)
    kap = np.float32(kappa)
    if kap == 0:
        s = hard.astype(T)
    else:
        inv2k = T(np.float32(1.0 / (2.0 * np.float64(kap))))
        s = np.clip((T(0.5) + (m * inv2k).astype(T)).astype(T), T(0), T(1))
    return hard, p, d, s


def columns(view, gaits=TABLE, dtype=np.float64):
    """[n, 10] clock columns of a view (phi, g, freq).  float64: sin / cos of 2 pi p; float32: NumPy's sin / cos of f32(2 pi) * p."""
    T = dtype
    _, p, d, _ = foot_quantities(view["phi"], view["g"], gaits, 0.0, T)
    arg = (T(2.0 * np.pi) * p).astype(T)
    return np.concatenate([np.sin(arg).astype(T), np.cos(arg).astype(T), np.asarray(view["freq"], np.float32).astype(T)[:, None], d[:, None]], 1)


def weight_vector(weights, dtype=np.float64):
    return S.weight_vector(weights, TERMS, dtype)


def evaluate(view, body_force, feet, done=None, command=None, reward=None, base=None, *, gaits=TABLE, weights=WEIGHTS, kappa=KAPPA,
             sigma_force, sigma_velocity, swing_height_target, min_command_speed, force_threshold=FORCE_THRESHOLD, dtype=np.float64, **_):
    """The terms of the view `view` (the old episode's, after its advance) on the rows the sensor reports for the state: body_force
    [n, 13, 3], feet [n, 4, 12] (float32).  Returns a dict: hard, s, contact [n, 4]; terms [n, 4] (unweighted, finished envs NOT
    zeroed), components [n, 4], shaped [n], reward_out [n], wide [n, C0 + 4]."""
    T = dtype
    f32 = lambda v: T(np.float32(v))
    force, rows = np.asarray(body_force, np.float32), np.asarray(feet, np.float32)
    n = len(rows)
    hard, _, _, s = foot_quantities(view["phi"], view["g"], gaits, kappa, T)
    if command is not None:
        cmd = np.asarray(command, np.float32)
        stand = np.maximum(np.abs(cmd[:, 0]), np.abs(cmd[:, 1])) <= np.float32(min_command_speed)
        hard, s = hard | stand[:, None], np.where(stand[:, None], T(1), s)
    F, v, z = force[:, list(FEET)].astype(T), rows[..., VEL].astype(T), rows[..., POS_Z].astype(T)
    sq = lambda a: ((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]).astype(T) + a[..., 2] * a[..., 2]).astype(T)
    inv_sf2 = f32(1.0 / (np.float64(np.float32(sigma_force)) ** 2))
    inv_sv2 = f32(1.0 / (np.float64(np.float32(sigma_velocity)) ** 2))
    swing, lift = (T(1) - s).astype(T), (z - f32(swing_height_target)).astype(T)
    per_foot = [(swing * (T(1) - np.exp((-sq(F) * inv_sf2).astype(T)).astype(T)).astype(T)).astype(T),
                (s * (T(1) - np.exp((-sq(v) * inv_sv2).astype(T)).astype(T)).astype(T)).astype(T),
                (swing * (lift * lift).astype(T)).astype(T)]
    contact = force[:, list(FEET), 2] > np.float32(force_threshold)             # exact f32 comparison
    terms = np.zeros((n, NTERMS), T)
    for j, a in enumerate(per_foot):
        acc = a[:, 0]
        for f in range(1, 4):                                     # ascending f
            acc = (acc + a[:, f]).astype(T)
        terms[:, j] = acc
    terms[:, 3] = (contact == hard).sum(1)
    return dict(S.tail(terms, weights, TERMS, done, reward, base, T), hard=hard, s=s, contact=contact, terms=terms)


def term_tolerance(terms64, margin=1.0):
    return S.term_tolerance(terms64, TERMS, BUDGET_TERM, margin)


def component_tolerance(ref, weights=WEIGHTS, margin=1.0):
    """[n, 4]: the terms' bounds times |w_k|, and the one rounding of f32(w_k x term_k)."""
    return S.component_tolerance(ref, weights, TERMS, BUDGET_TERM, margin)


def reward_tolerance(ref, weights=WEIGHTS, reward=None, margin=1.0):
    return S.reward_tolerance(ref, weights, TERMS, BUDGET_TERM, BUDGET_SUM_ULPS, reward, margin)


def clock_tolerance(margin=1.0):
    """[10]: the sin / cos columns within margin x E_clock; freq and d exact."""
    return np.array([margin * BUDGET_CLOCK] * 8 + [0.0, 0.0])


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def check_columns(what, cols, view):
    """[n, 10] clock columns against a view: freq and d exact, sin / cos within MARGIN x E_clock."""
    ref = columns(view)
    assert _same(cols[:, 8:], ref[:, 8:].astype(np.float32)), what
    err = np.abs(cols[:, :8].astype(np.float64) - ref[:, :8])
    assert (err <= clock_tolerance(MARGIN)[:8]).all(), (what, err.max())
    return float(err.max())


# ---- the states, extras and the scripted done table ---------------------------------------------------------------------------------------
def fixture_states(fix):
    """67 indices into tests/golden/contact_cells.npz: 48 states built on a foot's sample points (12 per foot: the foot stands) and 19
    built on other bodies (most feet in the air), interleaved so that every prefix (1, 5) mixes them."""
    body, kind = np.asarray(fix["body"]), np.asarray(fix["kind"])
    on_foot = [np.flatnonzero((body == b) & (kind == 0)) for b in FEET]
    feet = np.stack([idx[np.linspace(0, len(idx) - 1, 12).astype(int)] for idx in on_foot], 1).ravel()       # foot 0, 1, 2, 3, 0, ...
    others = np.flatnonzero(~np.isin(body, FEET))
    others = others[np.linspace(0, len(others) - 1, 19).astype(int)]
    out, a, b = [], list(feet), list(others)
    while a or b:
        out += a[:5] + b[:2]
        a, b = a[5:], b[2:]
    out = np.array(out)
    assert len(out) == 67 and len(set(out.tolist())) == 67
    return out


def extras(n, seed=21):
    """(done [n] bool, command [n, 2] f32, reward [n] f32, base [n, 11] f32): every tenth env finished; commands on both sides of
    min_command_speed and some exactly on it (those stand)."""
    rng = np.random.default_rng(seed)
    done = np.arange(n) % 10 == 7
    command = rng.uniform(-0.3, 0.3, (n, 2)).astype(np.float32)
    command[::9] = (np.float32(LIMITS["min_command_speed"]), np.float32(-0.05))
    command[4::9] = (np.float32(0.02), np.float32(-0.01))
    reward = rng.normal(0.0, 2.0, n).astype(np.float32)
    base = rng.normal(0.0, 1.0, (n, C0)).astype(np.float32)
    return done, command, reward, base


def done_table(n, steps=STEPS):
    """[steps][n] uint8; row t - 1 is env-step t.  By env index mod 5: 0 never finishes, 1 finishes at step 1, 2 at step 7, 3 at step
    23, 4 at steps 1, 7, 23 and 40."""
    done = np.zeros((steps, n), np.uint8)
    i = np.arange(n)
    for t, groups in ((1, (1, 4)), (7, (2, 4)), (23, (3, 4)), (40, (4,))):
        if t <= steps:
            done[t - 1] = np.isin(i % 5, groups)
    return done


def obs_rows(n, width, steps=STEPS, tag=0):
    """[steps][n][width] f32, the same for every caller."""
    return np.random.default_rng(2000 + tag).standard_normal((steps, n, width)).astype(np.float32)
