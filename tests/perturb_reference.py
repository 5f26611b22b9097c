"""The perturbation layer's definitions (include/quadgym.h: qg_perturb_*) in NumPy -- the integers exactly, everything after them in
float64 -- and the inputs the CPU and GPU tests share: the moment samples, the scripted `done` table, the shapes, the rows.

Nothing here touches the library: tests/test_perturb_reference.py holds this module against the oracle's hash and against the
moments a standard normal must have, tests/test_zz_perturb_gpu.py holds the kernels against this module."""
import functools

import numpy as np

U64 = np.uint64
SALT = 0x51474E4F49534531
C_STREAM, C_ENV, C_COUNTER = 0xA0761D6478BD642F, 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
NJ = 12


def _u64(x):
    """A Python int (reduced mod 2^64) or an integer array as a uint64 array of at least one dimension (array arithmetic wraps)."""
    if isinstance(x, (int, np.integer)):
        return np.array([int(x) % (1 << 64)], dtype=U64)
    return np.atleast_1d(np.asarray(x)).astype(U64)


def _mix64(x):
    x = x ^ (x >> U64(30))
    x = x * U64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> U64(27))
    x = x * U64(0x94D049BB133111EB)
    return x ^ (x >> U64(31))


def k_int(seed, env, episode, stream, salted=True):
    """k(s): the 24-bit integer behind uniform24s(seed_p, env, episode, s); the arguments broadcast.  salted=False leaves the seed as
    it is (the simulator's own streams: what the oracle's qgo_uniform_stream hashes)."""
    seed_p = _u64(int(seed) + (SALT if salted else 0))
    x = seed_p + U64(C_STREAM) * _u64(stream) + U64(C_ENV) * (_u64(env) + U64(1)) + U64(C_COUNTER) * (_u64(episode) + U64(1))
    return (_mix64(_mix64(x)) >> U64(40)).astype(np.int64)


def bias_stream(c):
    return 2 + 2 * np.asarray(c, dtype=np.int64)


def frame_stream(f, q):
    return 4096 + 2 * (128 * np.asarray(f, dtype=np.int64) + np.asarray(q, dtype=np.int64))


def z64(seed, env, episode, stream):
    """z(s) in float64."""
    s = np.asarray(stream, dtype=np.int64)
    u1 = (k_int(seed, env, episode, s) + 1).astype(np.float64) / 2.0 ** 24
    u2 = k_int(seed, env, episode, s + 1).astype(np.float64) / 2.0 ** 24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def z32(seed, env, episode, stream):
    """z(s) as written, every operation in float32 (NumPy's): the yardstick of the error budget E_z."""
    s = np.asarray(stream, dtype=np.int64)
    f = np.float32
    u1 = (k_int(seed, env, episode, s) + 1).astype(f) * f(2.0 ** -24)
    u2 = k_int(seed, env, episode, s + 1).astype(f) * f(2.0 ** -24)
    return np.sqrt(f(-2.0) * np.log(u1)) * np.cos(f(2.0 * np.pi) * u2)


def delay_of(seed, env, episode, lo, hi):
    return lo + ((k_int(seed, env, episode, 0) * (hi - lo + 1)) >> 24)


# -- the moment samples -------------------------------------------------------------------------------------------------------------
MOMENT_SEEDS = (0, 1, 12345)
MOMENT_EPISODES = (0, 1, 7)
MOMENT_ENVS, MOMENT_FRAMES, MOMENT_COLS = 16, 64, 26
BIAS_ENVS = 1024
DELAY_ENVS, DELAY_RANGE = 4096, (0, 3)


def obs_sample(seed, episode, z=z64):
    """[16 envs][64 frames][26 columns] of z(S(f, c))."""
    e, f, c = np.ix_(np.arange(MOMENT_ENVS), np.arange(MOMENT_FRAMES), np.arange(MOMENT_COLS))
    return z(seed, e, episode, frame_stream(f, c))


def action_sample(seed, episode, z=z64):
    """[16 envs][64 ages][12 joints] of z(S(f, 64 + j))."""
    e, f, j = np.ix_(np.arange(MOMENT_ENVS), np.arange(MOMENT_FRAMES), np.arange(NJ))
    return z(seed, e, episode, frame_stream(f, 64 + j))


def bias_sample(seed, episode, z=z64):
    """[1024 envs][26 columns] of z(2 + 2c)."""
    e, c = np.ix_(np.arange(BIAS_ENVS), np.arange(MOMENT_COLS))
    return z(seed, e, episode, bias_stream(c))


def lag1(x, axis):
    """Lag-1 autocorrelation along an axis, about the sample's mean and variance."""
    x = np.asarray(x, dtype=np.float64)
    d = x - x.mean()
    a = np.take(d, range(0, x.shape[axis] - 1), axis=axis)
    b = np.take(d, range(1, x.shape[axis]), axis=axis)
    return float((a * b).mean() / d.var())


def moment_report(x):
    """What the moment bounds are about: `(|mean|, |std - 1|, largest |lag-1 correlation| over the axes)` and the sample's N.  The
    bounds: 4 / sqrt(N) for the mean and the correlations, 4 / sqrt(2N) for the standard deviation (four standard errors each)."""
    x = np.asarray(x, dtype=np.float64)
    corr = max(abs(lag1(x, ax)) for ax in range(x.ndim))
    return abs(float(x.mean())), abs(float(x.std()) - 1.0), corr, x.size


def assert_moments(x, what):
    mean, dstd, corr, n = moment_report(x)
    assert mean <= 4.0 / np.sqrt(n), (what, "mean", mean, n)
    assert corr <= 4.0 / np.sqrt(n), (what, "lag-1 correlation", corr, n)
    assert dstd <= 4.0 / np.sqrt(2.0 * n), (what, "std", dstd, n)
    return mean, dstd, corr


@functools.lru_cache(maxsize=None)
def error_budget():
    """E_z: the largest deviation of the float32 NumPy evaluation of z from the float64 one over the moment samples (the draws the
    tests use)."""
    worst = 0.0
    for seed in MOMENT_SEEDS:
        for ep in MOMENT_EPISODES:
            for sample in (obs_sample, action_sample, bias_sample):
                worst = max(worst, float(np.abs(sample(seed, ep, z32).astype(np.float64) - sample(seed, ep, z64)).max()))
    return worst


# -- the scripted run ---------------------------------------------------------------------------------------------------------------
STEPS = 12
SHAPES = ((5, 3, 4), (67, 10, 26), (64, 1, 33))             # (n, window, frame_dim)
DELAYS = ((0, (0, 0)), (3, (0, 3)), (3, (2, 2)))           # (max_delay, (lo, hi))
RESET_ACTION = tuple(np.float32(v) for v in (0.0, 0.0, -0.5) * 4)


def done_table(n, steps=STEPS):
    """[steps][n] uint8; row t - 1 is env-step t.  By env index mod 5: 0 never finishes, 1 finishes at step 1, 2 at step 5, 3 at step
    12, 4 at steps 1, 5 and 12."""
    done = np.zeros((steps, n), np.uint8)
    i = np.arange(n)
    for t, groups in ((1, (1, 4)), (5, (2, 4)), (12, (3, 4))):
        if t <= steps:
            done[t - 1] = np.isin(i % 5, groups)
    return done


def column_stds(frame_dim):
    """(obs_std, bias_std) f32: every third column is left alone, one column has noise only, one bias only."""
    c = np.arange(frame_dim)
    obs = np.where(c % 3 == 2, 0.0, 0.01 + 0.004 * c).astype(np.float32)
    bias = np.where(c % 3 == 2, 0.0, 0.02 + 0.001 * c).astype(np.float32)
    obs[0], bias[min(1, frame_dim - 1)] = 0.0, 0.0
    return obs, bias


def rows(n, width, steps=STEPS, tag=0):
    """[steps][n][width] f32 of mixed magnitude, the same for every caller."""
    rng = np.random.default_rng(1000 + tag)
    return (rng.standard_normal((steps, n, width)) * rng.choice([0.01, 1.0, 30.0], (steps, n, width))).astype(np.float32)


class Checker:
    """The layer in float64 with exact integers.  The methods return what the kernels must produce (`ref`), the noise term alone
    (`e`) for the rounding part of the tolerance, and the (episode, top frame) every row was given."""

    def __init__(self, n, frame_dim, window=1, max_delay=0, delays=(0, 0), action_std=0.0, obs_std=None, bias_std=None,
                 reset_action=RESET_ACTION, done_row="terminal", seed=0, env_index_base=0):
        self.n, self.F, self.W, self.M = n, frame_dim, window, max_delay + 1
        self.lo, self.hi = delays
        self.action_std = float(np.float32(action_std))
        zeros = np.zeros(frame_dim, np.float32)
        self.obs_std = np.asarray(zeros if obs_std is None else obs_std, np.float32).astype(np.float64)
        self.bias_std = np.asarray(zeros if bias_std is None else bias_std, np.float32).astype(np.float64)
        self.reset_action = np.asarray(reset_action, np.float32)
        self.done_row, self.seed = done_row, seed
        self.env = env_index_base + np.arange(n, dtype=np.int64)
        self.age, self.episode = np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.ring = np.zeros((self.M, n, NJ), np.float32)

    def delays(self):
        return delay_of(self.seed, self.env, self.episode, self.lo, self.hi)

    def noise(self, episode, top):
        """e(f, c) of the rows (episode[i], top[i]): [n][window][frame_dim] float64."""
        k = np.arange(self.W)
        f = np.maximum(top[:, None] - (self.W - 1 - k)[None, :], 0)                     # [n][W]
        c = np.arange(self.F)
        zb = z64(self.seed, self.env[:, None], episode[:, None], bias_stream(c)[None, :])                          # [n][F]
        zo = z64(self.seed, self.env[:, None, None], episode[:, None, None], frame_stream(f[:, :, None], c[None, None, :]))
        return self.bias_std * zb[:, None, :] + self.obs_std * zo

    def perturb_actions(self, actions):
        """-> (ref [n][12] float64, v [n][12] float32: the delayed rows before the noise, e [n][12] float64)."""
        a, d, i = self.age, self.delays(), np.arange(self.n)
        self.ring[a % self.M, i] = actions
        v = np.where((a - d >= 0)[:, None], self.ring[(a - d) % self.M, i], self.reset_action[None, :]).astype(np.float32)
        j = np.arange(NJ)
        e = self.action_std * z64(self.seed, self.env[:, None], self.episode[:, None], frame_stream(a[:, None], 64 + j[None, :]))
        return v.astype(np.float64) + e, v, e

    def observe(self, obs, done, terminal=None):
        """-> dict: ref / e of the rows ([n][W * F] float64), term_ref / term_e likewise (rows of finished envs only are meaningful),
        episode and top of every row."""
        fin = np.asarray(done).astype(bool)
        a1 = self.age + 1
        reset = fin & (self.done_row == "reset")
        ep_row, top_row = np.where(reset, self.episode + 1, self.episode), np.where(reset, 0, a1)
        e = self.noise(ep_row, top_row).reshape(self.n, -1)
        out = {"ref": np.asarray(obs, np.float64) + e, "e": e, "episode": ep_row, "top": top_row}
        if terminal is not None:
            te = self.noise(self.episode, a1).reshape(self.n, -1)
            out.update(term_ref=np.asarray(terminal, np.float64) + te, term_e=te)
        self.episode = self.episode + fin
        self.age = np.where(fin, 0, a1)
        return out

    def begin(self, mask=None, rows=None):
        sel = np.ones(self.n, bool) if mask is None else np.asarray(mask).astype(bool)
        self.episode = self.episode + sel
        self.age = np.where(sel, 0, self.age)
        if rows is None:
            return None
        e = self.noise(self.episode, np.zeros(self.n, np.int64)).reshape(self.n, -1)
        return {"ref": np.where(sel[:, None], np.asarray(rows, np.float64) + e, np.asarray(rows, np.float64)), "e": np.where(sel[:, None], e, 0.0)}


def tolerance(std_sum, x, e):
    """The bound of the GPU parity check: 4 E_z (obs_std[c] + bias_std[c]) for the f32 evaluation of z, 2^-23 (|in| + |e|) for the
    roundings of the products, their sum and the final add."""
    return 4.0 * error_budget() * std_sum + 2.0 ** -23 * (np.abs(x) + np.abs(e))
