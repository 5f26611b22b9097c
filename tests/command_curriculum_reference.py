"""The definition of the command curriculum (include/quadgym.h, "command curriculum") in NumPy: bins, weights, counts, segments and the
inverse CDF in exact integers -- k(s) is tests/perturb_reference.py's, in the curriculum's key space --, the edges, speed, alpha, theta
and the criteria's sums in float32 in the stated order, the six command floats in float64; the parameters and the scripted table of
done and components rows the CPU and GPU tests share, and the float32 budget measured by tests/test_command_curriculum_reference.py.
No GPU, no torch."""
import numpy as np

import perturb_reference as P

SALT = 0x5147434D44435531                                         # "QGCMDCU1"
MAX_CRITERIA = 4
PI32 = np.float32(np.pi)

# ---- the parameters the tests share ----------------------------------------------------------------------------------------------------
N_COLUMNS = 7                                                     # columns of the scripted components rows
CRITERIA = ((2, 1, 0.5), (5, -1, 0.25))                           # (column, sense, threshold): column 2's mean >= 0.5, column 5's <= 0.25
# the 3 x 4 grid of the scripted table: one unlocked bin, (si, ai) = (0, 0)
MAIN = dict(speed=(0.1, 1.0), bins=(3, 4), initial_weights=(12,) + (0,) * 11, weight_max=12, delta=5, resample_steps=6, min_steps=3,
            criteria=CRITERIA, fixed_heading=0.75, seed=7, env_index_base=1000)
ONE = dict(speed=(0.3, 0.3), bins=(1, 1), initial_weights=(1,), weight_max=3, delta=1, resample_steps=0, min_steps=1, criteria=(),
           fixed_heading=None, seed=1, env_index_base=0)
WIDE = dict(speed=(0.0, 2.0), bins=(16, 16), initial_weights=tuple(int(b % 17 == 0) * 9 for b in range(256)), weight_max=65536, delta=4096,
            resample_steps=4, min_steps=2, criteria=CRITERIA[:1], fixed_heading=None, seed=12345, env_index_base=1 << 33)
SIZES = {"main": 300, "one": 70, "wide": 300}                     # 300: two blocks of 256 envs, the last wave partial
STEPS = 30

# ---- the measured float32 budget (tests/test_command_curriculum_reference.py prints a fresh measurement and fails if it exceeds these) --
# The largest deviation of the float32 evaluation of the six command floats (NumPy's float32 sin / cos, every product and sum rounded)
# from the float64 evaluation of the SAME float32 (speed, alpha, theta), over 2^16 draws of the 16 x 16 grid with speeds up to 2, as
# |c32 - c64| <= atol x scale, scale = 1 for the heading and max(speed, 2^-126) for the two velocities.
# Where the sizes come from.  sin and cos of a float32 angle up to pi are within an ulp of 1 of the exact value, 6e-8, and the
# heading is that.  A velocity component is speed x (sin or cos): the factor's 6e-8 and one rounding of the product, another 6e-8
# relative.  A global velocity component is a difference (or sum) of two such products of three factors: three roundings and two factor
# errors per product, and one more rounding of the sum: up to 2 x (3 + 2) x 6e-8 + 6e-8 = 6.6e-7 of the speed.
# measured: heading 6.81e-8 (share 0.68), velocity 9.16e-8 x speed (0.65), global velocity 1.71e-7 x speed (0.66)
BUDGET_COMMAND = {"velocity": 1.4e-7, "heading": 1.0e-7, "global_velocity": 2.6e-7}
MARGIN = 4.0          # a different but equally valid rounding order and sincosf, as tests/gait_schedule_reference.py


# ---- exact integers -----------------------------------------------------------------------------------------------------------------------
def k(seed, env, segment, stream):
    """k(s) of the curriculum's key space: perturb_reference's hash with seed + SALT and the segment as the episode."""
    return P.k_int(int(seed) + SALT, env, segment, stream, salted=False)


def draw_bin(k0, weights):
    """The bin of the 24-bit draws `k0` (array) under integer `weights`: r = (k0 * T) >> 24, the smallest b with cumsum_b > r."""
    cum = np.cumsum(np.asarray(weights, np.int64))
    r = (np.asarray(k0, np.int64) * cum[-1]) >> 24
    return np.searchsorted(cum, r, side="right").astype(np.int64)


def bin_counts(weights):
    """How many of the 2^24 values of k(0) fall in each bin, arithmetically: k0 gives r iff ceil(r 2^24 / T) <= k0 < ceil((r + 1) 2^24 / T),
    so bin b, which holds r in [cum_{b-1}, cum_b), gets ceil(cum_b 2^24 / T) - ceil(cum_{b-1} 2^24 / T) of them."""
    cum = [0] + [int(c) for c in np.cumsum(np.asarray(weights, np.int64))]
    T = cum[-1]
    first = [-((-c << 24) // T) for c in cum]                     # ceil(c 2^24 / T)
    return np.array([b - a for a, b in zip(first, first[1:])], np.int64)


def neighbours(c, n_speed, n_alpha):
    """N(c) as a sorted list: c, its speed neighbours (no wrap), its angle neighbours (wrap) -- a set."""
    si, ai = divmod(int(c), n_alpha)
    out = {c}
    if si > 0:
        out.add((si - 1) * n_alpha + ai)
    if si < n_speed - 1:
        out.add((si + 1) * n_alpha + ai)
    out.add(si * n_alpha + (ai + 1) % n_alpha)
    out.add(si * n_alpha + (ai - 1) % n_alpha)
    return sorted(out)


# ---- float32 in the stated order -----------------------------------------------------------------------------------------------------------
def widths(speed, bins):
    """(ws, wa) float32: formed in float64, rounded once."""
    lo, hi = np.float32(speed[0]), np.float32(speed[1])
    return np.float32((np.float64(hi) - np.float64(lo)) / int(bins[0])), np.float32(2.0 * np.pi / int(bins[1]))


def edges(speed, bins):
    """(speed_edges [n_speed + 1], alpha_edges [n_alpha + 1]) float32: one product and one add each."""
    ws, wa = widths(speed, bins)
    f32 = np.float32
    s = [f32(f32(speed[0]) + f32(f32(si) * ws)) for si in range(int(bins[0]) + 1)]
    a = [f32(-PI32 + f32(f32(ai) * wa)) for ai in range(int(bins[1]) + 1)]
    return np.array(s, f32), np.array(a, f32)


def commands64(speed, alpha, theta):
    """[n, 6] float64: (vx, vy, hx, hy, gvx, gvy) of float32 (speed, alpha, theta)."""
    sp, al, th = (np.asarray(x, np.float32).astype(np.float64) for x in (speed, alpha, theta))
    vx, vy, hx, hy = sp * np.cos(al), sp * np.sin(al), np.cos(th), np.sin(th)
    return np.stack([vx, vy, hx, hy, hx * vx - hy * vy, hy * vx + hx * vy], axis=1)


def commands32(speed, alpha, theta):
    """The same in float32, every product and sum rounded: what the budget is measured on."""
    f32 = np.float32
    sp, al, th = (np.asarray(x, f32) for x in (speed, alpha, theta))
    ca, sa, ct, st = np.cos(al).astype(f32), np.sin(al).astype(f32), np.cos(th).astype(f32), np.sin(th).astype(f32)
    vx, vy = (sp * ca).astype(f32), (sp * sa).astype(f32)
    gx = ((ct * vx).astype(f32) - (st * vy).astype(f32)).astype(f32)
    gy = ((st * vx).astype(f32) + (ct * vy).astype(f32)).astype(f32)
    return np.stack([vx, vy, ct, st, gx, gy], axis=1)


def command_tolerance(speed, margin=1.0):
    """[n, 6]: the budget of each command float at the speeds `speed`."""
    scale = np.maximum(np.abs(np.asarray(speed, np.float64)), 2.0 ** -126)
    B = BUDGET_COMMAND
    return margin * np.stack([B["velocity"] * scale] * 2 + [np.full_like(scale, B["heading"])] * 2 + [B["global_velocity"] * scale] * 2, axis=1)


def _ordered(x):
    """float32 bits as integers that order like the values (-0 = +0); NaN has no place: callers mask it."""
    b = np.asarray(x, np.float32).view(np.uint32).astype(np.int64)
    b = np.where((b & 0x7FFFFFFF) == 0, 0, b)
    return np.where(b & 0x80000000, -(b & 0x7FFFFFFF), b)


class Curriculum:
    """n envs of the curriculum.  `advance(done, components)` and `begin(mask)` move the state on as the launches do; `bin`, `steps`,
    `segment`, `sum`, `weight`, `episodes`, `successes` are the state, `speed`, `alpha`, `theta` (float32) the running segments' draws."""

    def __init__(self, n, speed, bins, initial_weights, weight_max, delta, resample_steps, min_steps, criteria, fixed_heading, seed,
                 env_index_base):
        self.n, self.range, self.shape, self.B = n, speed, (int(bins[0]), int(bins[1])), int(bins[0]) * int(bins[1])
        self.W, self.delta, self.R, self.min_steps = int(weight_max), int(delta), int(resample_steps), int(min_steps)
        self.criteria, self.fixed_heading, self.seed = tuple(criteria), fixed_heading, seed
        self.env = int(env_index_base) + np.arange(n, dtype=np.int64)
        self.weight = np.array(initial_weights[:self.B], np.int64)
        self.episodes, self.successes = np.zeros(self.B, np.int64), np.zeros(self.B, np.int64)
        self.bin, self.steps, self.segment = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.sum = np.zeros((MAX_CRITERIA, n), np.float32)
        self.speed, self.alpha, self.theta = (np.zeros(n, np.float32) for _ in range(3))
        self.ws, self.wa = widths(speed, bins)
        self._draw(np.ones(n, bool))

    def _draw(self, sel):
        """A new draw for the envs of `sel` from the weights as they stand, with their segment counters as they stand."""
        f32 = np.float32
        i = np.flatnonzero(sel)
        env, seg = self.env[i], self.segment[i]
        b = draw_bin(k(self.seed, env, seg, 0), self.weight)
        si, ai = b // self.shape[1], b % self.shape[1]
        u = [k(self.seed, env, seg, s).astype(f32) * f32(2.0 ** -24) for s in (1, 2, 3)]
        edge_s = (f32(self.range[0]) + (si.astype(f32) * self.ws).astype(f32)).astype(f32)
        edge_a = (-PI32 + (ai.astype(f32) * self.wa).astype(f32)).astype(f32)
        self.bin[i] = b
        self.speed[i] = (edge_s + (self.ws * u[0]).astype(f32)).astype(f32)
        self.alpha[i] = (edge_a + (self.wa * u[1]).astype(f32)).astype(f32)
        if self.fixed_heading is None:
            self.theta[i] = (PI32 * ((f32(2) * u[2]).astype(f32) - f32(1)).astype(f32)).astype(f32)
        else:
            self.theta[i] = f32(self.fixed_heading)
        self.steps[i] = 0
        self.sum[:, i] = 0

    def commands(self):
        """[n, 6] float64 of the running segments."""
        return commands64(self.speed, self.alpha, self.theta)

    def advance(self, done, components):
        """Returns what the launch decided: ended, success [n] bool, by_done [n] bool (the segment ended because done named it), the
        successes per bin of this launch [B] and the weights before it."""
        fin = np.zeros(self.n, bool) if done is None else np.asarray(done) != 0
        self.steps = self.steps + 1
        for j, (column, _, _) in enumerate(self.criteria):
            with np.errstate(invalid="ignore"):
                self.sum[j] = (self.sum[j] + np.asarray(components, np.float32)[:, column]).astype(np.float32)
        ended = fin | (self.steps == self.R)
        success = ended & (self.steps >= self.min_steps)
        for j, (_, sense, threshold) in enumerate(self.criteria):
            bound = (np.float32(threshold) * self.steps.astype(np.float32)).astype(np.float32)
            nan = np.isnan(self.sum[j]) | np.isnan(bound)
            a, b = _ordered(np.where(nan, 0, self.sum[j])), _ordered(np.where(nan, 0, bound))
            success &= ~nan & ((a >= b) if sense > 0 else (a <= b))
        np.add.at(self.episodes, self.bin[ended], 1)
        s_b = np.bincount(self.bin[success], minlength=self.B).astype(np.int64)
        self.successes += s_b
        before = self.weight.copy()
        gain = np.array([sum(int(s_b[b]) for b in neighbours(c, *self.shape)) for c in range(self.B)], np.int64)
        self.weight = np.minimum(self.W, before + self.delta * gain)
        self.segment = self.segment + ended
        self._draw(ended)
        return dict(ended=ended, success=success, by_done=fin, s_b=s_b, before=before)

    def begin(self, mask=None):
        sel = np.ones(self.n, bool) if mask is None else np.asarray(mask) != 0
        self.segment = self.segment + sel
        self._draw(sel)
        return sel


# ---- the scripted table ---------------------------------------------------------------------------------------------------------------------
SHORT, EARLY, LOW = 1, 2, 3                                       # env classes by index mod 10
NAN_ROWS = ((2, 14, 2), (8, 35, 5))                               # (env-step, env, column) of the NaN entries: envs of no class


def table(n, steps=STEPS):
    """(done [steps][n] uint8, components [steps][n][N_COLUMNS] float32); row t - 1 is env-step t.  By env index mod 10:
      1  done at env-steps 2, 12, 22: with min_steps = 3 a segment of 2 steps that meets every criterion, and fails;
      2  done at env-steps 4, 14, 24: a segment ended by done that is long enough;
      3  column 2 stays near 0: its segments fail the first criterion;
    every other env's columns meet both criteria, but for the NaN entries of NAN_ROWS, each inside a segment that would succeed."""
    rng = np.random.default_rng(4242)
    i = np.arange(n)
    done = np.zeros((steps, n), np.uint8)
    for t in range(1, steps + 1):
        done[t - 1] = ((i % 10 == SHORT) & (t % 10 == 2)) | ((i % 10 == EARLY) & (t % 10 == 4))
    comps = rng.normal(0.0, 0.05, (steps, n, N_COLUMNS)).astype(np.float32)
    comps[:, :, 2] += np.where(i % 10 == LOW, 0.0, 1.0).astype(np.float32)
    for t, env, column in NAN_ROWS:
        if env < n and t <= steps:
            comps[t - 1, env, column] = np.nan
    return done, comps
