"""One whole PPO iteration as INTEGRATION.md section 13 lists it -- step / normalise / record, last values, GAE, gather, advantage
normalisation, loss and gradient, gradient-norm clipping, Adam, update_from, begin -- composed from the float64 checkers of the single
handles (normalize_reference, policy_reference, rollout_buffer_reference, ppo_reference), and the auditor of a recorded run of that loop.
No new maths.  NumPy only: tests/test_ppo_iteration_reference.py (CPU) and tests/test_ppo_iteration_gpu.py share it.

The environment is a set of tables, so every input is known on the host: per step a float32 raw observation row ``[n, D]`` (column c has
scale ``logspace(-1, 1, D)[c]`` and an offset of up to three scales, so the normaliser has work to do), a done column (Bernoulli 5 %)
and the policy's ``eps``.  The one thing the "env" computes is the raw reward of the row it emits,
``-mean_a (action - 0.5 tanh(raw_obs[:, :A]))^2``.  No truncation bootstrap.

The order of a run is the listing's: a first observation (a step with zero actions, ``pre``), ``begin``, one warm-up ``step()`` (the one
the listing runs before it captures the graph, ``warm``), ``begin`` again, then per iteration K steps (``roll``), the critic on slot K,
GAE, the minibatches, ``begin()``.

``audit`` is teacher-forced: every stage is checked in float64 against the recording's OWN inputs to that stage, so an error does not
compound and nothing chaotic enters; it returns findings and never leaves a stage out."""
import collections
import math
import os

import numpy as np

import normalize_reference as NR
import policy_reference as PR
import ppo_reference as G
import rollout_buffer_reference as RB

GAMMA, GAE_LAMBDA = 0.99, 0.95
CLIP_RANGE, ENT_COEF, VF_COEF, MAX_GRAD_NORM = 0.2, 0.0, 0.5, 0.5
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
DONE_RATE = 0.05
STORED = ("observations", "actions", "log_probs", "values", "rewards", "dones", "advantages", "returns")
FIELDS = G.Batch._fields        # observations, actions, old_values, old_log_prob, advantages, returns: SB3's RolloutBufferSamples
FIELD_SOURCE = {"observations": "observations", "actions": "actions", "old_values": "values", "old_log_prob": "log_probs",
                "advantages": "advantages", "returns": "returns"}
STAGES = ("normaliser", "forward", "storage", "last_values", "gae", "gather", "gradient", "first_minibatch", "parameters", "episodes")

Case = collections.namedtuple("Case", ["name", "n", "K", "D", "A", "hidden", "out_tanh", "clip_range_vf", "iterations", "epochs",
                                       "batch_size", "learning_rate", "seed", "perm_seed"])
# The smallest shapes that still cross a wave, a tile, a partial-sum slot and both copy paths of the buffer:
# plain: n = 131 is two waves and three lanes; D = 33 takes the 4-byte row path and the packed stride 35; 1048 samples in minibatches of
#        600 (two slots, 512 + 88 = five tiles and a half) and 448 (28 tiles, after a larger call)
# wide:  D = 260 takes the 16-byte row path; out_tanh and value clipping on; 350 samples in minibatches of 200 and 150, ragged last tiles
# The seeds (of the tables, and of the device generator whose permutations device_permutations() holds) were found by search against
# the census of tests/test_ppo_iteration_reference.py: census() below over 10 table seeds x 24 generator seeds; DESIGN.md section 4.12.
CASES = {
    "plain": Case("plain", 131, 8, 33, 12, (64, 64), False, None, 2, 2, 600, 3e-4, 7, 13),
    "wide": Case("wide", 70, 5, 260, 7, (32, 48), True, 0.3, 2, 2, 200, 3e-4, 3, 7),
}
# one deliberate wiring error each -> the stage of audit() that must report it
MISWIRES = collections.OrderedDict([
    ("no_begin", "storage"),                      # no begin() between iterations: every add of iteration 2 overflows
    ("last_values_slot", "last_values"),          # the critic run on slot K - 1
    ("swap_old_fields", "gradient"),              # old_log_prob and old_values change places on the way into ppo_grad
    ("advantages_before_compute", "gather"),      # the advantages gathered are those from before compute()
    ("stale_forward", "forward"),                 # the forward passes of iteration 2 use the parameters of the start of iteration 1
    ("grad_one_behind", "gradient"),              # ppo_grad reads the parameters of one update_from earlier
    ("returns_first_permutation", "gather"),      # the second epoch gathers `returns` with the first epoch's permutation
])

Finding = collections.namedtuple("Finding", ["stage", "where", "what"])
Tables = collections.namedtuple("Tables", ["raw_pre", "done_pre", "eps_warm", "raw", "done", "eps", "perms", "flat0"])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def tables(case):
    """Every input of a run, float32 (uint8 dones, int64 permutations), from the case's seed: two raw rows before the first rollout
    (the first observation and the warm-up step's), then ``[iterations, K]`` rows; the initial parameters (torch.nn.Linear's
    default initialisation, ``log_std`` around log 0.3: ppo_reference.make_net)."""
    rng = np.random.default_rng([case.seed, case.n, case.K, case.D, case.A])
    n, K, D, A, I = case.n, case.K, case.D, case.A, case.iterations
    scale = np.logspace(-1.0, 1.0, D)
    offset = rng.uniform(-3.0, 3.0, D) * scale

    def rows(*lead):
        return (offset + scale * rng.standard_normal(lead + (n, D))).astype(np.float32)
    raw_pre, raw = rows(2), rows(I, K)
    done_pre = (rng.random((2, n)) < DONE_RATE).astype(np.uint8)
    done = (rng.random((I, K, n)) < DONE_RATE).astype(np.uint8)
    eps_warm = rng.standard_normal((n, A)).astype(np.float32)
    eps = rng.standard_normal((I, K, n, A)).astype(np.float32)
    perms = np.stack([np.stack([rng.permutation(K * n) for _ in range(case.epochs)]) for _ in range(I)]).astype(np.int64)
    perms = device_permutations(case, perms)
    actor, log_std, critic = G.make_net(rng, D, case.hidden, A, value=True)
    t = Tables(raw_pre, done_pre, eps_warm, raw, done, eps, perms, PR.flatten(actor, log_std, critic))
    for a in t:
        a.setflags(write=False)
    return t


PERMUTATIONS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppo_iteration_perms.npz")


def device_permutations(case, default=None):
    """``[iterations, epochs, K n]``: what ``buf.get(generator=g)`` draws pass after pass on the device for ``g =
    torch.Generator("cuda").manual_seed(case.perm_seed)`` -- ``torch.randperm`` on the GPU, which the CPU cannot restate, so the two
    committed cases' draws were recorded once on an MI355X (tests/golden/ppo_iteration_perms.npz) and the GPU test asserts that the
    device still draws them: the census of the float64 loop then holds for the minibatches the device forms.  A case without a
    record (the simulator's, whose one full batch per rollout needs no census) keeps ``default``."""
    with np.load(PERMUTATIONS) as z:
        key = f"{case.name}_seed{case.perm_seed}"
        if key not in z.files:
            return default
        perms = z[key].astype(np.int64).reshape(case.iterations, case.epochs, case.K * case.n)
    return perms


def toy_reward(raw_obs, actions, A):
    """The raw reward of the row the toy env emits, in the dtype of ``actions``."""
    dt = actions.dtype
    return -np.mean((actions - dt.type(0.5) * np.tanh(raw_obs[:, :A].astype(dt))) ** 2, axis=1)


def unflatten(flat, case):
    """``(actor, log_std, critic)`` views of a canonical flat vector (policy_reference.flatten's order)."""
    flat = np.asarray(flat)
    off, towers = 0, []
    for out_dim in (case.A, 1):
        layers = []
        for o, i in PR.tower_shapes(case.D, case.hidden, out_dim):
            layers.append((flat[off:off + o * i].reshape(o, i), flat[off + o * i:off + o * i + o]))
            off += o * i + o
        towers.append(layers)
        if out_dim == case.A:
            log_std = flat[off:off + case.A]
            off += case.A
    assert off == flat.size
    return towers[0], log_std, towers[1]


def tensor_slices(case):
    """``[(name, offset, size)]`` of the parameter tensors in the canonical order (FusedMlpPolicy.param_layout's names)."""
    out, off = [], 0
    for tower, out_dim in (("actor", case.A), ("critic", 1)):
        for k, (o, i) in enumerate(PR.tower_shapes(case.D, case.hidden, out_dim)):
            out += [(f"{tower}.{k}.weight", off, o * i), (f"{tower}.{k}.bias", off + o * i, o)]
            off += o * i + o
        if tower == "actor":
            out.append(("log_std", off, case.A))
            off += case.A
    return out


# ---- the record of a run --------------------------------------------------------------------------------------------------------------
class Recording:
    """Host arrays of one run of the loop; everything that crosses a seam is recorded once.

    ``steps``: one dict per env-step in time order -- ``kind`` (pre / warm / roll), ``iteration``, ``t``, ``raw_obs``, ``raw_reward``,
    ``done`` (what the env left), ``norm_obs``, ``norm_reward`` (what the normaliser made of it), ``norm_state`` (the statistics it
    reports after the step) and, but for ``pre``, ``eps``,
    ``actions``, ``log_prob``, ``value`` and ``params`` (the flat parameters the policy reports at that step).
    ``iterations``: one dict each -- ``storage`` (the eight tensors after compute), ``last_values``, ``last_params``, ``info``,
    ``episode_stats`` (episodes, length_sum, return_sum) and ``minibatches``: dicts of ``epoch``, ``idx``, the six
    gathered fields, ``adv_norm``, ``params`` (reported before ppo_grad), ``grad``, ``stats``, ``flat_before``, ``flat_after``,
    ``params_after`` (reported after update_from)."""

    def __init__(self, case):
        self.case = case.name
        self.initial_params = None
        self.steps, self.iterations = [], []

    def arrays(self):
        """Every recorded value as ``(path, ndarray)``, in a fixed order: what a bit-for-bit comparison of two runs walks."""
        def walk(path, obj):
            if isinstance(obj, dict):
                for k in sorted(obj):
                    yield from walk(f"{path}.{k}", obj[k])
            elif isinstance(obj, (list, tuple)):
                for k, v in enumerate(obj):
                    yield from walk(f"{path}[{k}]", v)
            elif isinstance(obj, str):
                yield path, np.frombuffer(obj.encode(), np.uint8)
            else:
                yield path, np.asarray(obj)
        yield from walk("initial_params", self.initial_params)
        yield from walk("steps", self.steps)
        yield from walk("iterations", self.iterations)


def differences(a, b):
    """Paths at which two recordings differ in shape, dtype or any bit."""
    out = []
    xs, ys = list(a.arrays()), list(b.arrays())
    if [p for p, _ in xs] != [p for p, _ in ys]:
        return ["the recordings do not hold the same entries"]
    for (p, x), (_, y) in zip(xs, ys):
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            out.append(p)
    return out


# ---- the loop in NumPy ----------------------------------------------------------------------------------------------------------------
def normalize_advantages(adv):
    """SB3's normalize_advantage in the dtype of ``adv``: torch's ``std()`` is the unbiased one."""
    return (adv - adv.mean()) / (adv.std(ddof=1) + adv.dtype.type(1e-8))


def run_numpy(case, dtype=np.float64, miswire=None):
    """The loop on the case's tables.  ``float64``: the reference run (the normaliser's outputs stay the float32 values its checker
    defines).  ``float32``: every value that crosses a seam -- stored rows, the forward pass's outputs, the gradient, the parameters --
    is rounded to float32, GAE, advantage normalisation, clipping and Adam run in float32 arithmetic, and each kernel's own stage is
    computed in float64 and rounded once: a device whose kernels round correctly, which plays the device's part on a machine
    without one.  ``miswire`` is one key of ``MISWIRES``; the recording then holds what the handles WOULD REPORT (the current
    parameters, the gathered rows), not what the wrong wire carried."""
    assert miswire is None or miswire in MISWIRES
    dt = np.dtype(dtype)
    n, K, D, A = case.n, case.K, case.D, case.A
    T = tables(case)

    def rd(x):
        return np.asarray(x, np.float64).astype(dt)
    rec = Recording(case)
    flat = T.flat0.astype(dt)
    rec.initial_params = flat.copy()
    pol = flat.copy()                         # what update_from last gave the policy
    pol_behind = flat.copy()                  # ... and the time before
    m, v, adam_t = np.zeros_like(flat), np.zeros_like(flat), 0
    nz = NR.Normalizer(n, D, gamma=GAMMA)
    buf = RB.RolloutBuffer(n, K, D, A, GAMMA, GAE_LAMBDA)
    rows = {}

    def env_and_norm(entry, raw_obs, done, actions):
        reward = toy_reward(raw_obs, actions, A)
        obs_n, rew_n = nz.step(raw_obs, reward, done)
        entry.update(raw_obs=raw_obs.copy(), raw_reward=reward, done=done.copy(), norm_obs=obs_n, norm_reward=rew_n, norm_state=nz.state())
        rows["obs"] = obs_n

    def step(kind, it, t, raw_obs, done, eps):
        used = T.flat0.astype(dt) if (miswire == "stale_forward" and kind == "roll" and it == 1) else pol
        actor, log_std, critic = unflatten(used, case)
        _, act, lp, val = PR.forward(actor, log_std, rows["obs"], eps=eps, critic=critic, out_tanh=case.out_tanh)
        entry = dict(kind=kind, iteration=it, t=t, eps=eps.copy(), actions=rd(act), log_prob=rd(lp), value=rd(val), params=pol.copy())
        env_and_norm(entry, raw_obs, done, entry["actions"])
        buf.add(entry["norm_obs"], entry["actions"], entry["log_prob"], entry["value"], entry["norm_reward"], done,
                episode_reward=entry["raw_reward"])
        rec.steps.append(entry)

    first = dict(kind="pre", iteration=-1, t=0)
    env_and_norm(first, T.raw_pre[0], T.done_pre[0], np.zeros((n, A), dt))
    rec.steps.append(first)
    buf.begin(rows["obs"])
    step("warm", -1, 0, T.raw_pre[1], T.done_pre[1], T.eps_warm)
    buf.begin(rows["obs"])

    for it in range(case.iterations):
        for t in range(K):
            step("roll", it, t, T.raw[it, t], T.done[it, t], T.eps[it, t])
        actor, log_std, critic = unflatten(pol, case)
        slot = K - 1 if miswire == "last_values_slot" else K
        last_values = rd(PR.mlp(critic, buf.obs[slot], False)[:, 0])
        adv_before = buf.advantages.copy()
        F = buf.pos
        a, r = RB.gae(rd(buf.rewards[:F]), rd(buf.values[:F]), buf.dones[:F], last_values, GAMMA, GAE_LAMBDA)
        buf.advantages[:F], buf.returns[:F] = a, r
        entry = dict(storage={"observations": rd(buf.obs), "actions": rd(buf.actions), "log_probs": rd(buf.log_prob),
                              "values": rd(buf.values), "rewards": rd(buf.rewards), "dones": buf.dones.copy(),
                              "advantages": rd(buf.advantages), "returns": rd(buf.returns)},
                     last_values=last_values, last_params=pol.copy(), info=dict(pos=buf.pos, overflow=buf.overflow, bad_index=buf.bad_index),
                     minibatches=[])
        total = buf.pos * n
        for epoch in range(case.epochs):
            perm = T.perms[it, epoch]
            for start in range(0, total, case.batch_size):
                idx = perm[start:start + case.batch_size]
                got = {k: rd(a) for k, a in buf.gather(idx).items()}
                if miswire == "advantages_before_compute":
                    got["advantages"] = rd(adv_before.reshape(-1)[idx])
                if miswire == "returns_first_permutation" and epoch == 1:
                    got["returns"] = rd(buf.returns.reshape(-1)[T.perms[it, 0][start:start + case.batch_size]])
                adv_norm = normalize_advantages(got["advantages"])
                batch = G.Batch(**got)._replace(advantages=adv_norm)
                used = batch._replace(old_values=batch.old_log_prob, old_log_prob=batch.old_values) if miswire == "swap_old_fields" else batch
                a_, ls_, c_ = unflatten(pol_behind if miswire == "grad_one_behind" else pol, case)
                stats, grad = G.loss_and_grad(a_, ls_, c_, used, case.out_tanh, CLIP_RANGE, case.clip_range_vf, ENT_COEF, VF_COEF)
                grad = rd(grad)
                mb = dict(epoch=epoch, idx=idx.copy(), adv_norm=adv_norm, params=pol.copy(), grad=grad.copy(),
                          stats=rd([stats[k] for k in G.STAT_NAMES] + [0.0, 0.0]), flat_before=flat.copy(), **got)
                # torch.nn.utils.clip_grad_norm_ and torch.optim.Adam, in the loop's dtype
                coef = min(dt.type(1.0), dt.type(MAX_GRAD_NORM) / (np.sqrt(np.sum(grad * grad)) + dt.type(1e-6)))
                g = grad * coef
                adam_t += 1
                m = dt.type(BETA1) * m + dt.type(1 - BETA1) * g
                v = dt.type(BETA2) * v + dt.type(1 - BETA2) * g * g
                denom = np.sqrt(v) / dt.type(math.sqrt(1 - BETA2 ** adam_t)) + dt.type(ADAM_EPS)
                flat = flat - dt.type(case.learning_rate / (1 - BETA1 ** adam_t)) * (m / denom)
                pol_behind, pol = pol, flat.copy()
                mb.update(flat_after=flat.copy(), params_after=pol.copy())
                entry["minibatches"].append(mb)
        if miswire != "no_begin":
            buf.begin()
        ret_sum, length_sum, episodes = buf.episode_stats(clear=True)
        entry["episode_stats"] = dict(episodes=episodes, length_sum=length_sum, return_sum=ret_sum)
        rec.iterations.append(entry)
    return rec


# ---- the auditor ----------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _norm_output(out, x, mean, var, epsilon, clip):
    """The rule of tests/test_normalize_gpu.py::test_outputs_within_one_ulp_and_clipped_exactly: nothing beyond the clip, elements
    whose float64 quotient lies beyond it exactly at it, every other within one float32 ulp.  Returns (ok, largest error in ulp)."""
    ref = NR.apply_f64(x, mean, var, epsilon)
    over = np.abs(ref) > clip * (1 + 1e-6)
    ok = bool(np.all(np.abs(out) <= np.float32(clip))) and np.array_equal(out[over], (np.sign(ref[over]) * clip).astype(np.float32))
    refc = np.clip(ref, -clip, clip)
    err = float((np.abs(out.astype(np.float64) - refc) / NR.ulp32(refc)).max())
    return ok and err <= 1.0, err


def _norm_statistics(got, ref, seen, ret_seen):
    """The rule of tests/test_normalize_gpu.py::_check_statistics -- counts equal, |d mean| <= 1e-12 max|x| and |d var| <= 1e-9 var +
    (1e-12 max|x|)^2 per column (max|x| over everything the column has seen), the returns and their statistic within 1e-12 of the
    largest |return| -- as the largest error over its bound (inf for a count that differs)."""
    if got["obs_rms.count"] != ref["obs_rms.count"] or got["ret_rms.count"] != ref["ret_rms.count"]:
        return math.inf
    m_tol = 1e-12 * seen
    v_tol = 1e-9 * ref["obs_rms.var"] + m_tol ** 2
    dm, dv = np.abs(got["obs_rms.mean"] - ref["obs_rms.mean"]), np.abs(got["obs_rms.var"] - ref["obs_rms.var"])
    fm = np.divide(dm, m_tol, out=np.where(dm > 0, np.inf, 0.0), where=m_tol > 0)
    r_tol, rv_tol = 1e-12 * ret_seen, 1e-12 * min(ret_seen, ret_seen ** 2)
    dr = max(float(np.abs(got["returns"] - ref["returns"]).max()), abs(float(got["ret_rms.mean"] - ref["ret_rms.mean"])))
    drv = abs(float(got["ret_rms.var"] - ref["ret_rms.var"]))
    fr = max(dr / r_tol, drv / rv_tol) if ret_seen > 0 else (0.0 if dr == 0 and drv == 0 else math.inf)
    return max(float(fm.max()), float((dv / v_tol).max()), fr)


def audit(case, rec, grad_baseline, forward_baseline, forward_bound, report=None):
    """Findings of a float32 recording, stage by stage (``STAGES``); an empty list is a clean run.

    ``grad_baseline(actor, log_std, critic, batch, out_tanh, clip_range, clip_range_vf, ent_coef, vf_coef)`` returns torch float32
    autograd's ``(stats, [gradient per tensor])`` (ppo_torch.gradients with the dtype and device bound) and
    ``forward_baseline(actor, log_std, critic, obs, eps, out_tanh)`` the torch float32 modules' ``(actions, log_prob, value)``:
    the paths the kernels replace, on the same inputs.  ``forward_bound(torch_err, ref)`` is the tolerance rule of
    tests/test_policy_gpu.py.  ``report``, if given, is called with one line per minibatch (worst fused / torch / bound triple and
    the boundary gap) and one per stage with the largest ratio of an error to its bound."""
    n, K, D, A = case.n, case.K, case.D, case.A
    f64 = np.float64
    findings = []
    worst = collections.defaultdict(float)

    def find(stage, where, what):
        findings.append(Finding(stage, where, what))

    def note(stage, err, bound):
        worst[stage] = max(worst[stage], err / bound if bound > 0 else (0.0 if err == 0 else math.inf))

    if len(rec.iterations) != case.iterations or [s["kind"] for s in rec.steps] != ["pre", "warm"] + ["roll"] * (case.iterations * K):
        find("storage", "run", "the recording does not hold a first observation, a warm-up step and iterations x K steps")
        return findings
    roll = [[s for s in rec.steps if s["kind"] == "roll" and s["iteration"] == i] for i in range(case.iterations)]

    # -- normaliser: its reported statistics against the checker fed the recorded raw rows, its outputs against those statistics -------
    nz = NR.Normalizer(n, D, gamma=GAMMA)
    seen, ret_seen = np.zeros(D), 0.0
    for k, s in enumerate(rec.steps):
        ret_seen = max(ret_seen, float(np.abs(nz.returns * nz.gamma + s["raw_reward"].astype(f64)).max()))
        seen = np.maximum(seen, np.abs(s["raw_obs"].astype(f64)).max(0))
        nz.step(s["raw_obs"], s["raw_reward"], s["done"])
        err_s = _norm_statistics(s["norm_state"], nz.state(), seen, ret_seen)
        note("normaliser", err_s, 1.0)
        if not err_s <= 1.0:
            find("normaliser", f"step {k}", f"statistics at {err_s:.3g} of their bound, or a count that differs")
        sd = s["norm_state"]
        ok, err = _norm_output(s["norm_obs"], s["raw_obs"], sd["obs_rms.mean"], sd["obs_rms.var"], nz.epsilon, nz.clip_obs)
        ok_r, err_r = _norm_output(s["norm_reward"], s["raw_reward"], 0.0, sd["ret_rms.var"], nz.epsilon, nz.clip_reward)
        note("normaliser", max(err, err_r), 1.0)
        if not (ok and ok_r):
            find("normaliser", f"step {k}", f"observations {err:.3f} ulp, rewards {err_r:.3f} ulp, or a clipped element not at the clip")

    # -- forward: the recorded parameters on the observation in the slot the cursor stood on ------------------------------------------
    def check_forward(stage, where, params, obs, eps, got):
        actor, log_std, critic = unflatten(params, case)
        _, act, lp, val = PR.forward(actor, log_std, obs, eps=eps, critic=critic, out_tanh=case.out_tanh)
        t_act, t_lp, t_val = forward_baseline(actor, log_std, critic, obs, eps, case.out_tanh)
        for name, ref, tv in (("actions", act, t_act), ("log_prob", lp, t_lp), ("value", val, t_val)):
            if name not in got:
                continue
            err, terr = float(np.abs(got[name].astype(f64) - ref).max()), float(np.abs(np.asarray(tv, f64) - ref).max())
            bound = forward_bound(terr, ref)
            note(stage, err, bound)
            if not (np.isfinite(err) and err <= bound):
                find(stage, where, f"{name}: error {err:.3e}, torch float32 {terr:.3e}, bound {bound:.3e}")

    for i, it in enumerate(rec.iterations):
        obs = it["storage"]["observations"]
        for t, s in enumerate(roll[i]):
            check_forward("forward", f"iteration {i} step {t}", s["params"], obs[t], s["eps"], s)
    check_forward("forward", "warm-up step", rec.steps[1]["params"], rec.steps[0]["norm_obs"], rec.steps[1]["eps"], rec.steps[1])

    # -- storage: the per-step recordings bit for bit; slot 0 is the slot K of the iteration before -----------------------------------
    for i, it in enumerate(rec.iterations):
        st = it["storage"]
        if it["info"] != dict(pos=K, overflow=0, bad_index=0):
            find("storage", f"iteration {i}", f"info() = {it['info']}")
        before = rec.steps[1]["norm_obs"] if i == 0 else rec.iterations[i - 1]["storage"]["observations"][K]
        if not _same(st["observations"][0], before):
            find("storage", f"iteration {i}", "slot 0 is not the observation after the last step of the rollout before")
        for t, s in enumerate(roll[i]):
            for name, key in (("actions", "actions"), ("log_probs", "log_prob"), ("values", "value"), ("rewards", "norm_reward")):
                if not _same(st[name][t], s[key]):
                    find("storage", f"iteration {i} step {t}", f"{name} differs from what the step produced")
            if not _same(st["observations"][t + 1], s["norm_obs"]):
                find("storage", f"iteration {i} step {t}", "observations[t + 1] is not the normalised observation after the step")
            if not np.array_equal(st["dones"][t] != 0, s["done"] != 0) or st["dones"].dtype != np.uint8:
                find("storage", f"iteration {i} step {t}", "dones differ from what the env left")

    # -- last values: the critic at the current parameters on slot K --------------------------------------------------------------------
    for i, it in enumerate(rec.iterations):
        check_forward("last_values", f"iteration {i}", it["last_params"], it["storage"]["observations"][K], None, {"value": it["last_values"]})

    # -- GAE on the stored rewards, values, dones and the recorded last values ---------------------------------------------------------
    for i, it in enumerate(rec.iterations):
        st = it["storage"]
        a64, r64 = RB.gae(st["rewards"].astype(f64), st["values"].astype(f64), st["dones"], it["last_values"].astype(f64), GAMMA, GAE_LAMBDA)
        bound = RB.gae_bound(st["rewards"], st["values"], a64, GAMMA, GAE_LAMBDA)
        err = max(float(np.abs(st["advantages"] - a64).max()), float(np.abs(st["returns"] - r64).max()))
        note("gae", err, bound)
        if not err <= bound:
            find("gae", f"iteration {i}", f"error {err:.3e}, bound {bound:.3e}")

    # -- gather -------------------------------------------------------------------------------------------------------------------------
    total = K * n
    sizes = [min(case.batch_size, total - s) for s in range(0, total, case.batch_size)]
    for i, it in enumerate(rec.iterations):
        st, mbs = it["storage"], it["minibatches"]
        if [len(mb["idx"]) for mb in mbs] != sizes * case.epochs or [mb["epoch"] for mb in mbs] != [e for e in range(case.epochs) for _ in sizes]:
            find("gather", f"iteration {i}", f"minibatch sizes {[len(mb['idx']) for mb in mbs]}, expected {sizes} per epoch")
        for e in range(case.epochs):
            idx = np.concatenate([mb["idx"] for mb in mbs if mb["epoch"] == e] or [np.zeros(0, np.int64)])
            if not np.array_equal(np.sort(idx), np.arange(total)):
                find("gather", f"iteration {i} epoch {e}", "the index vectors are not a permutation of the filled samples")
        for j, mb in enumerate(mbs):
            for name in FIELDS:
                src = st[FIELD_SOURCE[name]]
                src = src[:K].reshape((total,) + src.shape[2:])
                if not _same(mb[name], src[mb["idx"]]):
                    find("gather", f"iteration {i} minibatch {j}", f"{name} is not the stored rows at the indices")

    # -- gradient and statistics at the recorded parameters and batch; first minibatch of every iteration -----------------------------
    slices = tensor_slices(case)
    kw = (CLIP_RANGE, case.clip_range_vf, ENT_COEF, VF_COEF)
    for i, it in enumerate(rec.iterations):
        for j, mb in enumerate(it["minibatches"]):
            where = f"iteration {i} minibatch {j}"
            actor, log_std, critic = unflatten(mb["params"], case)
            batch = G.Batch(*[mb[f] for f in FIELDS])._replace(advantages=mb["adv_norm"])
            gap = G.classes(actor, log_std, critic, batch, case.out_tanh, CLIP_RANGE, case.clip_range_vf)[3]
            if not gap >= G.BAND:
                find("gradient", where, f"a row lies {gap:.3e} from a clip boundary (at least {G.BAND:g} is required)")
            ref_stats, ref_grad = G.loss_and_grad(actor, log_std, critic, batch, case.out_tanh, *kw)
            t_stats, t_grads = grad_baseline(actor, log_std, critic, batch, case.out_tanh, *kw)
            if mb["grad"].shape != ref_grad.shape or not (np.isfinite(mb["grad"]).all() and np.isfinite(mb["stats"]).all()):
                find("gradient", where, "grad or stats of the wrong shape or not finite")
                continue
            top = (0.0, 0.0, 0.0, 1.0, "")
            for (name, off, size), tg in zip(slices, t_grads):
                ref, got = ref_grad[off:off + size], mb["grad"][off:off + size].astype(f64)
                scale = np.abs(ref).max()
                if scale == 0.0:
                    if np.any(got != 0.0):
                        find("gradient", where, f"{name}: the reference gradient is all zeros, the recorded one is not")
                    continue
                err, terr = float(np.abs(got - ref).max() / scale), float(np.abs(np.asarray(tg, f64).ravel() - ref).max() / scale)
                bound = max(4.0 * terr, 1e-6)
                note("gradient", err, bound)
                top = max(top, (err / bound, err, terr, bound, name))
                if not err <= bound:
                    find("gradient", where, f"{name}: error {err:.3e}, torch float32 {terr:.3e}, bound {bound:.3e}")
            for k, name in enumerate(G.STAT_NAMES):
                got = float(mb["stats"][k])
                if name == "clip_fraction":
                    if mb["stats"][k] != np.float32(ref_stats[name]):
                        find("gradient", where, f"clip_fraction {got:.6f}, reference {ref_stats[name]:.6f}")
                    continue
                err, terr = abs(got - ref_stats[name]), abs(t_stats[name] - ref_stats[name])
                bound = max(4.0 * terr, 1e-6)
                note("gradient", err, bound)
                top = max(top, (err / bound, err, terr, bound, name))
                if not err <= bound:
                    find("gradient", where, f"{name}: error {err:.3e}, torch float32 {terr:.3e}, bound {bound:.3e}")
            if mb["stats"][6] != 0 or mb["stats"][7] != 0:
                find("gradient", where, "stats[6:8] are not zero")
            if report:
                report(f"{case.name} {where} B={len(mb['idx'])}: worst {top[4]}: fused {top[1]:.3e} torch {top[2]:.3e} bound {top[3]:.3e}"
                       f"  clip_fraction {float(mb['stats'][5]):.4f}  boundary gap {gap:.3e}")
            if j == 0 and not (mb["stats"][5] == 0.0 and abs(float(mb["stats"][4])) <= 1e-6):
                find("first_minibatch", where, f"clip_fraction {float(mb['stats'][5]):.4f}, approx_kl {float(mb['stats'][4]):.3e}: the batch is "
                                               "not the rollout the current parameters collected")

    # -- parameters: what the policy reports is the optimiser's tensor, and it is what every later stage recorded ----------------------
    current = rec.initial_params
    if not _same(rec.steps[1]["params"], current):
        find("parameters", "warm-up step", "the policy does not report the initial parameters")
    for i, it in enumerate(rec.iterations):
        for t, s in enumerate(roll[i]):
            if not _same(s["params"], current):
                find("parameters", f"iteration {i} step {t}", "the forward pass's parameters are not those of the last update_from")
        if not _same(it["last_params"], current):
            find("parameters", f"iteration {i} last values", "the parameters are not those of the last update_from")
        for j, mb in enumerate(it["minibatches"]):
            where = f"iteration {i} minibatch {j}"
            if not _same(mb["params"], current) or not _same(mb["flat_before"], current):
                find("parameters", where, "ppo_grad's parameters, or the optimiser's tensor, are not those of the last update_from")
            if not _same(mb["params_after"], mb["flat_after"]):
                find("parameters", where, "params() after update_from differs from the optimiser's flat tensor")
            if _same(mb["flat_after"], mb["flat_before"]) or not np.isfinite(mb["flat_after"]).all():
                find("parameters", where, "the optimiser step changed nothing, or left a non-finite parameter")
            current = mb["flat_after"]

    # -- episode statistics: the checker's bookkeeping fed the recorded raw rewards and dones --------------------------------------------
    ref = RB.RolloutBuffer(n, K, D, A, GAMMA, GAE_LAMBDA)
    scale, k = 0.0, 1
    for i, it in enumerate(rec.iterations):
        while k < len(rec.steps) and rec.steps[k]["iteration"] <= i:
            s = rec.steps[k]
            ref.pos = 0                                     # the bookkeeping alone: the storage is checked above
            ref.add(s["norm_obs"], s["actions"], s["log_prob"], s["value"], s["norm_reward"], s["done"], episode_reward=s["raw_reward"])
            scale += float(np.abs(s["raw_reward"].astype(f64)).sum())
            k += 1
        ret_sum, length_sum, episodes = ref.episode_stats(clear=True)
        got = it["episode_stats"]
        err = abs(got["return_sum"] - ret_sum)
        note("episodes", err, 1e-12 * scale)
        if got["episodes"] != episodes or got["length_sum"] != length_sum or not err <= 1e-12 * scale:
            find("episodes", f"iteration {i}", f"{got}, expected episodes {episodes}, length_sum {length_sum}, return_sum {ret_sum!r}")

    if report:
        report(f"{case.name}: largest error / bound per stage: " + "  ".join(f"{s} {worst[s]:.3f}" for s in STAGES if s in worst))
    return findings


def census(case, rec):
    """Conditions on a float64 recording's inputs: the smallest distance of any minibatch's rows to a clip boundary (a value-clip
    boundary included when the case clips values), the clip fractions, the episodes finished per iteration and the overflow count."""
    gaps, fractions = [], []
    for it in rec.iterations:
        for mb in it["minibatches"]:
            actor, log_std, critic = unflatten(mb["params"], case)
            batch = G.Batch(*[mb[f] for f in FIELDS])._replace(advantages=mb["adv_norm"])
            gaps.append(float(G.classes(actor, log_std, critic, batch, case.out_tanh, CLIP_RANGE, case.clip_range_vf)[3]))
            fractions.append(float(mb["stats"][5]))
    return dict(min_gap=min(gaps), gaps=gaps, clip_fractions=fractions, episodes=[it["episode_stats"]["episodes"] for it in rec.iterations],
                overflow=max(it["info"]["overflow"] for it in rec.iterations))
