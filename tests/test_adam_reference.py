"""The float64 checker of the optimiser step (tests/adam_reference.py) against torch on the CPU, and the error budget the GPU tests of
tests/test_zz_adam_gpu.py use: how far the float32 evaluation of one step lies from the float64 evaluation of the same float32 inputs."""
import math

import numpy as np
import pytest
import torch

import adam_reference as A

from quadruped_gym_amd.policy import FusedMlpPolicy


def test_nets_straddle_the_norm_partition():
    slot = FusedMlpPolicy.ADAM_SLOT
    assert [A.n_params(k) for k in "ABC"] == [50, 13529, 332697]
    assert A.n_params("A") < slot and A.n_params("A") < 64
    for name in "BC":
        assert A.n_params(name) >= 3 * slot and A.n_params(name) % slot != 0
    g = A.make_gradient("B", 0, 50.0)
    assert np.count_nonzero(g == 0) >= A.n_params("B") // 16 and np.count_nonzero(np.abs(g) == np.float32(1e-12)) == A.n_params("B") // 16
    assert abs(float(np.sqrt(np.sum(g.astype(np.float64) ** 2))) - 50.0) < 1e-4


@pytest.mark.parametrize("mode", list(A.MODES))
def test_checker_equals_torch_float64(mode):
    """clip_grad_norm_ + torch.optim.Adam in float64 on the CPU, 20 steps: 1e-12 of the largest element of each vector."""
    norm, max_norm = A.MODES[mode]
    p = A.initial_params("B").astype(np.float64)
    m, v, t = np.zeros_like(p), np.zeros_like(p), 0
    flat = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([flat], lr=A.LR, betas=(A.BETA1, A.BETA2), eps=A.EPS)
    for k in range(20):
        g = A.make_gradient("B", k, norm).astype(np.float64)
        p, m, v, t, info = A.clip_and_adam(p, m, v, t, g, A.LR, A.BETA1, A.BETA2, A.EPS, max_norm, np.float64)
        flat.grad = torch.from_numpy(g.copy())
        if max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_([flat], max_norm)
            assert abs(float(total) - float(info["norm"])) <= 1e-12 * float(info["norm"])
        assert (float(info["coef"]) == 1.0) == (mode != "active")
        opt.step()
        state = opt.state[flat]
        for name, got, want in (("p", p, flat.detach().numpy()), ("m", m, state["exp_avg"].numpy()), ("v", v, state["exp_avg_sq"].numpy())):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (name, k)
    assert int(state["step"]) == t == 20


@pytest.mark.parametrize("n", [2, 17, 512, 65539])
def test_normalize_advantages_equals_torch(n):
    adv = np.random.default_rng(n).standard_normal(n) * 3.0 + 0.7
    t = torch.from_numpy(adv)
    want = ((t - t.mean()) / (t.std() + 1e-8)).numpy()
    assert np.abs(A.normalize_advantages(adv, np.float64) - want).max() <= 1e-12 * np.abs(want).max()
    want32 = ((t.float() - t.float().mean()) / (t.float().std() + 1e-8)).numpy()
    assert np.abs(A.normalize_advantages(adv.astype(np.float32), np.float32) - want32).max() <= 1e-5 * np.abs(want32).max()


def test_error_budget_is_within_the_committed_constants():
    worst = [0.0, 0.0, 0.0]
    for name in A.NETS:
        for t in A.BUDGET_STEPS:
            for mode in A.MODES:
                p, m, v, g, max_norm, ref = A.one_step_case(name, t, mode)
                _, m32, v32, _, info = A.clip_and_adam(p, m, v, t - 1, g, A.LR, A.BETA1, A.BETA2, A.EPS, max_norm, np.float32)
                assert m32.dtype == np.float32 and info["dp"].dtype == np.float32
                dev = A.deviations(m32, v32, info["dp"], ref)
                print(f"net {name} t {t:4d} {mode:8s}: m {dev[0]:.3f} ulp  v {dev[1]:.3f} ulp  |dp32 - dp64| / lr {dev[2]:.3e}")
                worst = [max(a, b) for a, b in zip(worst, dev)]
    print(f"measured budget: m {worst[0]:.3f} ulp, v {worst[1]:.3f} ulp, p {worst[2]:.3e}; committed: {A.BUDGET_M_ULP}, {A.BUDGET_V_ULP}, "
          f"{A.BUDGET_P:.3e}")
    assert worst[0] <= A.BUDGET_M_ULP and worst[1] <= A.BUDGET_V_ULP and worst[2] <= A.BUDGET_P
    # the constants are the measurement, rounded up: not a looser figure
    assert A.BUDGET_M_ULP <= 1.25 * worst[0] and A.BUDGET_V_ULP <= 1.25 * worst[1] and A.BUDGET_P <= 1.25 * worst[2]
    assert set(A.GPU_STEPS) <= set(A.BUDGET_STEPS)


def test_tolerances_follow_the_budget():
    p64, m64, v64 = np.array([0.5]), np.array([1.0]), np.array([3.0])
    tp, tm, tv = A.gpu_tolerances(p64, m64, v64)
    assert math.isclose(tp[0], 4 * A.BUDGET_P * A.LR + 0.5 * 2.0 ** -24)
    assert math.isclose(tm[0], max(4 * A.BUDGET_M_ULP, 1.0) * 2.0 ** -23) and math.isclose(tv[0], max(4 * A.BUDGET_V_ULP, 1.0) * 2.0 ** -22)
