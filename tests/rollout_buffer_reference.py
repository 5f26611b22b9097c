"""NumPy float64 restatement of the rollout buffer's semantics as include/quadgym.h states them (the qg_rollout_* section): the record of
a step with the truncation bootstrap, the per-env episode bookkeeping, GAE over a partial fill and the gather with zeroed bad rows.
Written from the header's formulas, not from anyone's source.  Also the shape table of the GPU tests and their input families."""
import numpy as np

# (K, n, obs_dim, act_dim): one env, envs on either side of a wave boundary (64, 65, 70, 83, 131), the 4-byte row path (obs_dim 1, 33,
# 26) and the 16-byte one (260, 512), the packed stride of 35 (obs_dim 33), K = 1 and K beyond the 16 steps of the unrolled load depth
SHAPES = [(1, 1, 1, 1), (3, 17, 33, 12), (5, 64, 26, 12), (4, 65, 260, 12), (37, 83, 33, 12), (8, 131, 512, 16), (64, 70, 33, 12)]
GAE_PARAMS = [(0.99, 0.95), (0.999, 1.0), (0.9, 0.0)]


class RolloutBuffer:
    """The buffer in float64 (the stored rows keep the f32 inputs' values exactly; rewards with a bootstrap are formed in f64 from
    f32(gamma), so they are the exact value the device rounds once)."""

    def __init__(self, n, K, obs_dim, act_dim, gamma=0.99, gae_lambda=0.95):
        self.n, self.K, self.D, self.A = n, K, obs_dim, act_dim
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.obs = np.zeros((K + 1, n, obs_dim))
        self.actions = np.zeros((K, n, act_dim))
        self.log_prob, self.values, self.rewards = np.zeros((K, n)), np.zeros((K, n)), np.zeros((K, n))
        self.advantages, self.returns = np.zeros((K, n)), np.zeros((K, n))
        self.dones = np.zeros((K, n), np.uint8)
        self.pos, self.overflow, self.bad_index = 0, 0, 0
        self.cur_return, self.cur_length = np.zeros(n), np.zeros(n, np.int64)
        self.fin_return, self.fin_length, self.fin_count = np.zeros(n), np.zeros(n, np.int64), np.zeros(n, np.int64)

    def begin(self, obs=None):
        self.obs[0] = self.obs[self.pos] if obs is None else np.asarray(obs, np.float64)
        self.pos = 0

    def add(self, next_obs, actions, log_prob, value, reward, done, trunc_value=None, episode_reward=None):
        p = self.pos
        if p == self.K:
            self.overflow += 1
            return
        done = np.asarray(done) != 0
        reward = np.asarray(reward, np.float64)
        self.actions[p], self.log_prob[p], self.values[p], self.dones[p] = actions, log_prob, value, done
        self.rewards[p] = reward if trunc_value is None else reward + np.float64(np.float32(self.gamma)) * np.asarray(trunc_value, np.float64)
        self.obs[p + 1] = next_obs
        self.cur_return += reward if episode_reward is None else np.asarray(episode_reward, np.float64)
        self.cur_length += 1
        self.fin_return[done] += self.cur_return[done]
        self.fin_length[done] += self.cur_length[done]
        self.fin_count[done] += 1
        self.cur_return[done], self.cur_length[done] = 0.0, 0
        self.pos = p + 1

    def compute(self, last_values):
        gae(self.rewards[:self.pos], self.values[:self.pos], self.dones[:self.pos], last_values, self.gamma, self.gae_lambda,
            self.advantages[:self.pos], self.returns[:self.pos])

    def gather(self, idx):
        idx = np.asarray(idx, np.int64)
        valid = self.pos * self.n
        ok = (idx >= 0) & (idx < valid)
        self.bad_index += int((~ok).sum())
        safe = np.where(ok, idx, 0)
        out = {}
        for name, a, w in (("observations", self.obs, self.D), ("actions", self.actions, self.A), ("old_values", self.values, 0),
                           ("old_log_prob", self.log_prob, 0), ("advantages", self.advantages, 0), ("returns", self.returns, 0)):
            flat = a.reshape(-1, w) if w else a.reshape(-1)
            rows = flat[safe].copy()
            rows[~ok] = 0.0
            out[name] = rows
        return out

    def episode_stats(self, clear=True):
        out = (float(np.sum(self.fin_return)), int(self.fin_length.sum()), int(self.fin_count.sum()))
        if clear:
            self.fin_return[:], self.fin_length[:], self.fin_count[:] = 0.0, 0, 0
        return out


def gae(rewards, values, dones, last_values, gamma, gae_lambda, advantages=None, returns=None):
    """The header's recurrence over the F = len(rewards) filled slots, in the dtype of `rewards` (float64 for the checker).  Returns
    (advantages, returns)."""
    F = rewards.shape[0]
    dt = rewards.dtype
    advantages = np.zeros_like(rewards) if advantages is None else advantages
    returns = np.zeros_like(rewards) if returns is None else returns
    a = np.zeros(rewards.shape[1:], dt)
    g, lam = dt.type(gamma), dt.type(gae_lambda)
    for t in range(F - 1, -1, -1):
        nnt = (1 - (np.asarray(dones[t]) != 0)).astype(dt)
        nv = np.asarray(last_values, dt) if t == F - 1 else values[t + 1]
        delta = rewards[t] + g * nv * nnt - values[t]
        a = delta + g * lam * nnt * a
        advantages[t] = a
        returns[t] = a + values[t]
    return advantages, returns


def gae_bound(rewards, values, adv64, gamma, gae_lambda):
    """8 * 2^-24 * M * S with M = max|r| + (1 + gamma) max|v| + gamma lambda max|A64| and S = sum_{j<F} (gamma lambda)^j."""
    F = rewards.shape[0]
    M = float(np.abs(rewards).max()) + (1.0 + gamma) * float(np.abs(values).max()) + gamma * gae_lambda * float(np.abs(adv64).max())
    S = float(np.sum((gamma * gae_lambda) ** np.arange(F)))
    return 8.0 * 2.0 ** -24 * M * S


# done patterns and value families of the GAE cases
GAE_CASES = ["no_done", "done_2pct", "done_20pct", "done_last", "all_done", "offset"]


def gae_inputs(case, K, n, seed=0):
    """f32 (rewards [K, n], values [K, n], dones u8 [K, n], last_values [n]) of one family: rewards N(0, 1), values 3 N(0, 1)."""
    rng = np.random.default_rng([seed, K, n, GAE_CASES.index(case)])
    r = rng.standard_normal((K, n)).astype(np.float32)
    v = (3.0 * rng.standard_normal((K, n))).astype(np.float32)
    lv = (3.0 * rng.standard_normal(n)).astype(np.float32)
    rate = {"no_done": 0.0, "done_2pct": 0.02, "done_20pct": 0.2, "done_last": 0.02, "all_done": 1.0, "offset": 0.02}[case]
    d = (rng.random((K, n)) < rate).astype(np.uint8)
    if case == "done_last":
        d[-1] = 1
    if case == "offset":
        r, v, lv = (r + 50.0).astype(np.float32), (v + 500.0).astype(np.float32), (lv + 500.0).astype(np.float32)
    return r, v, d, lv
