"""A whole PPO iteration on the GPU -- the training loop of INTEGRATION.md section 13 with RunningNormalizer.step_packed,
FusedMlpPolicy.forward / reserve_grad / ppo_grad / update_from, DeviceRolloutBuffer and torch's Adam on the one flat tensor -- recorded
and audited by tests/ppo_iteration_reference.py: every stage in float64 against the recording's own inputs to that stage.

No tolerance of its own: the normaliser's statistics and outputs by the rules of tests/test_normalize_gpu.py, the forward pass and the
last values by the rule of tests/test_policy_gpu.py (``bound`` of tests/policy_checks.py), GAE within gae_bound, stored and gathered rows and the
parameters bit for bit, the gradient and statistics by the rule of tests/test_ppo_gpu.py case 1 with torch float32 autograd on the
GPU as the yardstick, the first minibatch of an iteration by test_first_epoch_has_no_clipped_row, the episode statistics by
test_episode_statistics_equal_the_checker.
With QG_PPO_ITER_PARITY_OUT=<file> the audited runs append, per minibatch, the worst fused / torch / bound triple and the distance to
a clip boundary, and per run the largest error / bound of every stage (profiles/r16/ppo_iteration_parity.txt).

Streams: the module takes four from torch's pool, once, and uses all four (capture, graph-form loop, eager-form loop, the simulator's
graph-form loop), which leaves the tests that run later in the process the hardware-queue assignment they had."""
import functools
import os

import numpy as np
import pytest
import torch

import ppo_iteration_reference as P
import ppo_torch as T
from policy_checks import DEV, bound as forward_bound, torch_tower

from quadruped_gym_amd import _abi
from quadruped_gym_amd.normalize import RunningNormalizer
from quadruped_gym_amd.policy import FusedMlpPolicy
from quadruped_gym_amd.rollout import DeviceRolloutBuffer, RolloutBufferSamples
from quadruped_gym_amd.sim import BatchedSim

pytestmark = pytest.mark.gpu
CASE_NAMES = list(P.CASES)
# the simulator's loop: one update per rollout, so every ppo_grad call sees ratio 1 on all rows (0.2 from a clip boundary by construction)
SIM_CASE = P.Case("sim", 70, 6, 33, 12, (64, 64), False, None, 2, 1, 420, 3e-4, 11, 0)


@functools.lru_cache(maxsize=None)
def _streams():
    streams = [torch.cuda.Stream(DEV) for _ in range(4)]
    for s in streams:                                       # each one used once, whichever tests of this module run
        with torch.cuda.stream(s):
            torch.zeros(1, device=DEV)
        s.synchronize()
    return streams


def _report(line):
    print(line)
    out = os.environ.get("QG_PPO_ITER_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)            # a copy: the tables are read-only


def _h(t):
    return t.detach().cpu().numpy().copy()


# ---- the two envs: packed rows [n, D + 2] = obs | reward | done ---------------------------------------------------------------------------
class ToyEnv:
    """The table env of ppo_iteration_reference as torch ops: ``load`` copies the next raw row and done column into static buffers
    (outside a capture), ``step`` writes the packed row from them and the actions (capturable)."""

    def __init__(self, case):
        self.D, self.A = case.D, case.A
        self.raw, self.done = torch.zeros((case.n, case.D), device=DEV), torch.zeros(case.n, device=DEV)

    def load(self, raw, done):
        self.raw.copy_(raw)
        self.done.copy_(done)

    def step(self, acts, rows):
        rows[:, :self.D].copy_(self.raw)
        rows[:, self.D].copy_(-((acts - 0.5 * torch.tanh(self.raw[:, :self.A])) ** 2).mean(1))
        rows[:, self.D + 1].copy_(self.done)

    def close(self):
        pass


class SimEnv:
    """BatchedSim.step_device_packed with auto-reset and fall termination, as in tests/test_rollout_buffer_gpu.py's closed loop."""

    def __init__(self, case):
        task = _abi.default_task()
        task.auto_reset, task.use_fall, task.fall_height = 1, 1, 0.05
        self.sim = BatchedSim(case.n, task=task)
        self.sim.reset(seed=3)

    def load(self, raw, done):
        pass

    def step(self, acts, rows):
        self.sim.step_device_packed(acts, rows)

    def close(self):
        self.sim.close()


# ---- the loop of INTEGRATION.md section 13, recorded --------------------------------------------------------------------------------------
def run_device(case, env_type, form, loop_stream):
    """One run of the listing.  ``form`` is ``eager`` (``step()`` called K times) or ``graph`` (the listing's form: ONE ``step()``
    captured on a side stream and replayed K times, the tables' rows and ``eps`` copied into static buffers before each replay).
    Returns ``(Recording, slots)`` with ``slots[i]`` the slot ``buf.last_obs`` pointed at after rollout ``i``."""
    n, K, D, A = case.n, case.K, case.D, case.A
    tb = P.tables(case)
    d_raw_pre, d_done_pre, d_raw, d_done = _t(tb.raw_pre), _t(tb.done_pre).float(), _t(tb.raw), _t(tb.done).float()
    d_eps_warm, d_eps = _t(tb.eps_warm), _t(tb.eps)
    env = env_type(case)
    norm = RunningNormalizer(n, D, gamma=P.GAMMA)
    pol = FusedMlpPolicy(D, case.hidden, A, out_tanh=case.out_tanh, value=True)
    pol.set_params(tb.flat0)
    buf = DeviceRolloutBuffer(n, K, D, A, gamma=P.GAMMA, gae_lambda=P.GAE_LAMBDA)
    pol.reserve_grad(case.batch_size)
    flat = torch.from_numpy(pol.params()).to(DEV).requires_grad_(True)
    flat.grad, stats = torch.zeros_like(flat), torch.zeros(8, device=DEV)
    opt = torch.optim.Adam([flat], case.learning_rate)
    rows, seen = torch.zeros((n, D + 2), device=DEV), torch.zeros((n, D + 2), device=DEV)
    acts, logp, val = torch.zeros((n, A), device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    eps, raw = torch.zeros((n, A), device=DEV), torch.zeros(n, device=DEV)
    gen = torch.Generator(DEV).manual_seed(case.perm_seed)
    rec = P.Recording(case)
    rec.initial_params = pol.params()
    slots = []

    def env_and_norm():
        env.step(acts, rows)
        raw.copy_(rows[:, D])                               # the reward before normalisation, for ep_rew_mean
        seen.copy_(rows)                                    # (the whole raw row, for the record)
        norm.step_packed(rows)

    def step():
        pol.forward(rows[:, :D], acts, eps=eps, log_prob=logp, value=val)       # the observation in the buffer's current slot
        env_and_norm()
        buf.add_packed(rows, acts, logp, val, episode_reward=raw)

    def record(kind, it, t):
        torch.cuda.synchronize()
        entry = dict(kind=kind, iteration=it, t=t, raw_obs=_h(seen[:, :D]), raw_reward=_h(seen[:, D]), done=_h(seen[:, D + 1] != 0).astype(np.uint8),
                     norm_obs=_h(rows[:, :D]), norm_reward=_h(rows[:, D]), norm_state=norm.state_dict())
        if kind != "pre":
            entry.update(eps=_h(eps), actions=_h(acts), log_prob=_h(logp), value=_h(val), params=pol.params())
        rec.steps.append(entry)

    torch.cuda.synchronize()
    with torch.cuda.stream(loop_stream):
        env.load(d_raw_pre[0], d_done_pre[0])
        env_and_norm()                                      # a first observation (zero actions)
        record("pre", -1, 0)
        buf.begin(rows[:, :D])
        env.load(d_raw_pre[1], d_done_pre[1])
        eps.copy_(d_eps_warm)
        step()                                              # warm-up outside the capture
        record("warm", -1, 0)
        buf.begin(rows[:, :D])
    torch.cuda.synchronize()
    if form == "graph":
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=_streams()[0]):
            step()
        torch.cuda.synchronize()
    total = K * n
    for it in range(case.iterations):
        with torch.cuda.stream(loop_stream):
            for t in range(K):
                env.load(d_raw[it, t], d_done[it, t])
                eps.copy_(d_eps[it, t])
                if form == "graph":
                    graph.replay()                          # fills slot t: the cursor is read from and written to device memory
                else:
                    step()
                record("roll", it, t)
            slots.append(next(k for k in range(K + 1) if buf.observations[k].data_ptr() == buf.last_obs.data_ptr()))
            pol.forward(buf.observations[K], acts, value=val)                    # the critic on the observation after the last step
            buf.compute_returns_and_advantage(val)
            torch.cuda.synchronize()
            entry = dict(storage={name: _h(getattr(buf, name)) for name in P.STORED}, last_values=_h(val), last_params=pol.params(),
                         info=buf.info(), minibatches=[])
            for epoch in range(case.epochs):
                again = torch.Generator(DEV)
                again.set_state(gen.get_state())            # buf.get() draws one randperm(total) from `gen`: the same one from a copy
                perm = torch.randperm(total, device=DEV, generator=again)
                for j, batch in enumerate(buf.get(batch_size=case.batch_size, generator=gen)):
                    assert isinstance(batch, RolloutBufferSamples)
                    mb = dict(epoch=epoch, idx=_h(perm[j * case.batch_size:(j + 1) * case.batch_size]))
                    mb.update({name: _h(getattr(batch, name)) for name in P.FIELDS})
                    adv = batch.advantages                  # SB3's normalize_advantage
                    batch = batch._replace(advantages=(adv - adv.mean()) / (adv.std() + 1e-8))
                    mb.update(adv_norm=_h(batch.advantages), params=pol.params(), flat_before=_h(flat))
                    pol.ppo_grad(batch, flat.grad, stats, clip_range=P.CLIP_RANGE, clip_range_vf=case.clip_range_vf, ent_coef=P.ENT_COEF,
                                 vf_coef=P.VF_COEF)
                    mb.update(grad=_h(flat.grad), stats=_h(stats))
                    torch.nn.utils.clip_grad_norm_([flat], P.MAX_GRAD_NORM)
                    opt.step()
                    pol.update_from(flat)                   # the forward pass and the next ppo_grad see the new parameters
                    mb.update(flat_after=_h(flat), params_after=pol.params())
                    entry["minibatches"].append(mb)
            buf.begin()                                     # the next rollout continues from the last observation
            e = buf.episode_stats()
            entry["episode_stats"] = dict(episodes=e["episodes"], length_sum=e["length_sum"], return_sum=e["return_sum"])
            rec.iterations.append(entry)
    torch.cuda.synchronize()
    if form == "graph":
        del graph
    for h in (buf, pol, norm, env):
        h.close()
    return rec, slots


@functools.lru_cache(maxsize=None)
def _eager(name):
    """The toy env's eager run of a case, shared by the audit and the graph comparison; read-only."""
    rec, slots = run_device(P.CASES[name], ToyEnv, "eager", _streams()[2])
    for _, a in rec.arrays():
        a.setflags(write=False)
    return rec, slots


def _forward_baseline(actor, log_std, critic, obs, eps, out_tanh):
    """The path the forward pass replaces, as tests/test_policy_gpu.py forms it: torch float32 modules on the GPU."""
    with torch.no_grad():
        x = _t(np.asarray(obs, np.float32))
        mean = torch_tower([(np.array(W), np.array(b)) for W, b in actor], out_tanh)(x)
        std = _t(log_std).exp()
        act = mean if eps is None else mean + std * _t(eps)
        lp = torch.distributions.Normal(mean, std).log_prob(act).sum(-1)
        val = torch_tower([(np.array(W), np.array(b)) for W, b in critic], False)(x)[:, 0]
    return _h(act), _h(lp), _h(val)


def _audit(case, rec, report=None):
    return P.audit(case, rec, functools.partial(T.gradients, dtype=torch.float32, device=DEV), _forward_baseline, forward_bound, report=report)


def _all_finite(rec):
    return all(np.isfinite(a).all() for _, a in rec.arrays() if a.dtype.kind == "f")


# ---- 1. the audit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_audited_iteration(name):
    rec, slots = _eager(name)
    assert slots == [P.CASES[name].K] * P.CASES[name].iterations          # eagerly last_obs is the slot after the last step
    drawn = np.stack([np.concatenate([mb["idx"] for mb in it["minibatches"] if mb["epoch"] == e]) for it in rec.iterations for e in range(2)])
    # the census of tests/test_ppo_iteration_reference.py is taken on these permutations: should torch.randperm ever draw others,
    # record them anew (ppo_iteration_reference.device_permutations says how) and search the seeds again
    assert np.array_equal(drawn, P.tables(P.CASES[name]).perms.reshape(drawn.shape))
    findings = _audit(P.CASES[name], rec, report=_report)
    assert findings == [], findings[:10]


# ---- 2. the graph form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_graph_form_leaves_the_eager_forms_bits(name):
    eager, _ = _eager(name)
    graph, slots = run_device(P.CASES[name], ToyEnv, "graph", _streams()[1])
    assert P.differences(eager, graph) == []
    # the documented caveat: last_obs goes by the CALLER's count of add calls -- the one capture after begin(), none after begin()
    assert slots == [1] + [0] * (P.CASES[name].iterations - 1)


# ---- 3. the simulator in the loop ----------------------------------------------------------------------------------------------------------
def test_simulator_loop_two_iterations():
    case = SIM_CASE
    eager, _ = run_device(case, SimEnv, "eager", _streams()[2])
    graph, _ = run_device(case, SimEnv, "graph", _streams()[3])
    assert P.differences(eager, graph) == []
    assert _all_finite(eager)
    findings = _audit(case, eager)
    assert findings == [], findings[:10]
    for it in eager.iterations:
        assert len(it["minibatches"]) == 1 and len(it["minibatches"][0]["idx"]) == 420
        assert it["minibatches"][0]["stats"][5] == 0.0                              # ratio 1 on every row
    first, second = ([s for s in eager.steps if s["kind"] == "roll" and s["iteration"] == i] for i in (0, 1))
    assert not np.array_equal(first[0]["params"], second[0]["params"])            # the update reached the forward pass:
    assert not any(np.array_equal(a["actions"], b["actions"]) for a, b in zip(first, second))   # (the audit checked it at those parameters)
    print("episodes finished per iteration:", [it["episode_stats"]["episodes"] for it in eager.iterations])
