"""The float64 checker of the PPO loss and gradient pass (tests/ppo_reference.py) without a GPU: against torch float64 autograd of SB3's
formulae, and the census of the batches tests/test_ppo_gpu.py runs -- every clipping class is populated and no row sits on a boundary."""
import math

import numpy as np
import pytest

import ppo_reference as G
import ppo_torch as T


@pytest.mark.parametrize("value", [False, True])
@pytest.mark.parametrize("cv", [None, 0.3])
@pytest.mark.parametrize("out_tanh", [False, True])
@pytest.mark.parametrize("net", [(3, (16,), 1), (33, (64, 64), 12), (20, (16, 32, 240), 4)], ids=str)
def test_reference_equals_torch_float64_autograd(net, out_tanh, cv, value):
    rng = np.random.default_rng(5)
    actor, log_std, critic = G.make_net(rng, *net, value=value)
    batch = G.make_batch(rng, actor, log_std, critic, out_tanh, 300, 0.2, cv)
    stats, grad = G.loss_and_grad(actor, log_std, critic, batch, out_tanh, 0.2, cv, ent_coef=0.01, vf_coef=0.7)

    t_stats, want = T.gradients(actor, log_std, critic, batch, out_tanh, 0.2, cv, 0.01, 0.7)
    for name in G.STAT_NAMES:
        assert abs(stats[name] - t_stats[name]) <= 1e-10 * max(1.0, abs(t_stats[name])), name
    from quadruped_gym_amd.policy import FusedMlpPolicy
    layout = FusedMlpPolicy.param_layout(*net, value=value)
    assert len(want) == len(layout)
    for (name, (off, shape)), w in zip(layout.items(), want):
        got = grad[off:off + math.prod(shape)].reshape(shape)
        assert w.shape == shape and np.abs(w).max() > 0, name
        assert np.abs(got - w).max() <= 1e-10 * np.abs(w).max(), name


_BIG = [c for c in G.gradient_cases() if c.B >= 256]


@pytest.mark.parametrize("case", _BIG, ids=G.case_id)
def test_gpu_batches_populate_every_clipping_class(case):
    """Conditions on the inputs, not measurements of the kernel: with sigma = 0.3 about 13 % / 11 % / 32 % of the rows are expected in
    the clipped-high, clipped-low and value-clipped classes."""
    actor, log_std, critic, batch = G.build_case(case)
    hi, lo, vc, gap = G.classes(actor, log_std, critic, batch, case.out_tanh, 0.2, case.clip_range_vf)
    assert hi >= 0.04 and lo >= 0.04, (hi, lo)
    if critic and case.clip_range_vf:
        assert vc >= 0.10, vc
    assert gap >= G.BAND


def test_case_list_covers_the_options():
    cases = G.gradient_cases()
    assert len(_BIG) >= 15
    for net in G.NETS:
        mine = [c for c in cases if c.net == net]
        assert {c.B for c in mine} >= set(G.BATCHES)
        assert {c.out_tanh for c in mine} == {False, True} and {c.value for c in mine} == {False, True}
        assert {c.clip_range_vf for c in mine if c.value} == {None, 0.3}
    assert G.BATCHES[4] == G.SLOT_ROWS and G.BATCHES[5] == G.SLOT_ROWS + 1
    assert -(-G.BATCHES[6] // G.SLOT_ROWS) >= 3 and G.BATCHES[6] % G.SLOT_ROWS and G.BATCHES[6] % G.TILE_ROWS
