"""Float64 restatement of the running normaliser (include/quadgym.h, "running observation and reward normalisation"), written from
the formulae of SB3 2.x VecNormalize / RunningMeanStd and not from the kernels: the checker of tests/test_normalize_api.py and
tests/test_normalize_gpu.py.  NumPy only."""
import numpy as np

# (n, D) of the GPU tests and why each is there
SHAPES = (
    (1, 1),          # smallest case
    (1, 33),         # batch variance exactly 0
    (17, 33),        # through the packed stride 35, in place, done as float32
    (83, 26),        # a tail tile
    (83, 260),
    (83, 512),
    (4099, 260),     # a prime n: the partials of many workgroups and a ragged last one are combined whatever the tiling
)

COLUMN_KINDS = ("normal", "offset", "constant", "tiny", "uniform", "clipped")


def columns(rng, n, D, step=0):
    """Float32 ``[n, D]`` whose column c is of kind ``COLUMN_KINDS[c % 6]``: N(0, 1); 1000 + 0.1 N(0, 1); the constant 9.81;
    1e-6 N(0, 1); U(-3, 3); and N(0, 1) with, from ``step`` 4 on, a few entries (one in forty, at least one) of +-1000, which fall
    beyond the clip once the statistics have seen enough rows (an outlier among N rows lies at most sqrt(N) deviations out)."""
    x = np.empty((n, D), np.float64)
    for c in range(D):
        kind = COLUMN_KINDS[c % len(COLUMN_KINDS)]
        z = rng.standard_normal(n)
        if kind == "normal":
            col = z
        elif kind == "offset":
            col = 1000.0 + 0.1 * z
        elif kind == "constant":
            col = np.full(n, 9.81)
        elif kind == "tiny":
            col = 1e-6 * z
        elif kind == "uniform":
            col = rng.uniform(-3.0, 3.0, n)
        else:
            col = z
            if step >= 4:
                idx = rng.choice(n, size=max(1, n // 40), replace=False)
                col[idx] = 1000.0 * np.sign(z[idx])
        x[:, c] = col
    return x.astype(np.float32)


class RunningMeanStd:
    def __init__(self, shape=()):
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)
        self.count = 1e-4

    def update(self, batch):
        batch = np.asarray(batch, np.float64)
        n = batch.shape[0]
        bm, bv = batch.mean(axis=0), batch.var(axis=0)
        delta = bm - self.mean
        tot = self.count + n
        self.mean = self.mean + delta * n / tot
        M2 = self.var * self.count + bv * n + np.square(delta) * self.count * n / tot
        self.var = M2 / tot
        self.count = tot


def apply(x, mean, var, epsilon, clip):
    """Step 2 / 4 in float64, rounded to float32 at the very end."""
    y = (np.asarray(x, np.float64) - mean) / np.sqrt(var + epsilon)
    return np.clip(y, -clip, clip).astype(np.float32)


def apply_f64(x, mean, var, epsilon):
    """The unclipped, unrounded quotient (what the one-ulp rule of the GPU tests is measured against)."""
    return (np.asarray(x, np.float64) - mean) / np.sqrt(var + epsilon)


class Normalizer:
    def __init__(self, n_envs, obs_dim, gamma=0.99, epsilon=1e-8, clip_obs=10.0, clip_reward=10.0, norm_obs=True, norm_reward=True):
        self.n_envs, self.obs_dim = n_envs, obs_dim
        self.gamma, self.epsilon, self.clip_obs, self.clip_reward = gamma, epsilon, clip_obs, clip_reward
        self.norm_obs, self.norm_reward = norm_obs, norm_reward
        self.obs_rms, self.ret_rms = RunningMeanStd((obs_dim,)), RunningMeanStd(())
        self.returns = np.zeros(n_envs, np.float64)
        self.training = True

    def update_obs(self, obs):
        self.obs_rms.update(obs)

    def normalize_obs(self, obs):
        if not self.norm_obs:
            return np.asarray(obs, np.float32).copy()
        return apply(obs, self.obs_rms.mean, self.obs_rms.var, self.epsilon, self.clip_obs)

    def normalize_reward(self, reward):
        if not self.norm_reward:
            return np.asarray(reward, np.float32).copy()
        return apply(reward, 0.0, self.ret_rms.var, self.epsilon, self.clip_reward)

    def reset_returns(self):
        self.returns[:] = 0.0

    def step(self, obs, reward=None, done=None):
        """Steps 1 .. 5; returns ``(obs_out, reward_out)`` (``reward_out`` None for an observation-only step)."""
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        obs_out = self.normalize_obs(obs)
        if reward is None:
            return obs_out, None
        if self.training:
            self.returns = self.returns * self.gamma + np.asarray(reward, np.float64)
            self.ret_rms.update(self.returns)
        reward_out = self.normalize_reward(reward)
        if self.training and done is not None:
            self.returns[np.asarray(done) != 0] = 0.0
        return obs_out, reward_out

    def state(self):
        return {"obs_rms.mean": self.obs_rms.mean.copy(), "obs_rms.var": self.obs_rms.var.copy(), "obs_rms.count": np.float64(self.obs_rms.count),
                "ret_rms.mean": np.float64(self.ret_rms.mean), "ret_rms.var": np.float64(self.ret_rms.var),
                "ret_rms.count": np.float64(self.ret_rms.count), "returns": self.returns.copy()}


def ulp32(ref64):
    """One float32 ulp at the magnitude of each float64 reference value (the spacing of the binade it falls in)."""
    a = np.abs(np.asarray(ref64, np.float64)).astype(np.float32)
    a = np.maximum(a, np.float32(np.finfo(np.float32).tiny))
    return np.spacing(a).astype(np.float64)
