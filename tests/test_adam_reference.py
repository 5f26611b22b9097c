"""The float64 checker of the optimiser step (tests/adam_reference.py) against torch on the CPU, and the error budget the GPU tests of
tests/test_zz_adam_gpu.py use: how far the float32 evaluation of one step lies from the float64 evaluation of the same float32 inputs."""
import hashlib
import math

import numpy as np
import pytest
import torch

import adam_reference as A
import policy_backward_shapes as S
import policy_reference as R

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


# sha256 of initial_params(name) and of make_gradient(name, seed, norm) for (0, 50.0), (41, 1.0), (1001, 0.1), taken before the three
# functions learnt to take a description as well as a name: the named nets' arrays have not changed by a bit
_DIGESTS = {
    "A": (50, "a5a73936d83ffd847f02bc9d38e2b054b833d53098fd2768d59d5ec04eeaddba",
          "17e83ca8e635f2ee049201093c7347ddbe1af7febcb93c58a84370b934bce101", "b6c505aa5730846abf17800d780c1aba7bb5c969ef616a85f6ea2097c7cd913c",
          "e7ea010b693e55d6f394942737f0f9ee7d6bae0feee59704ad4588f1efca6ee1"),
    "B": (13529, "f93f6286c7813613e288ee93dbbfc4851f99e0c7911488e4b357be14b0546546",
          "1136acab6174e755345a98d4781f2cbbeeb535cd81e6af6d077b630ddb969a7f", "319d8705564bb6e8a214d951e304c13bd02d242305abd63863c173179c5a4390",
          "0264a2abeb958397f66c0733609af6b72c1389bb826b86966f751ed52957d87a"),
    "C": (332697, "07d78091227b5a66d728e485686521f48cce731d470a1f0749861ba08c266aaf",
          "b6c4c85180cfad2a01d7a43d2c3df075597e0c67892ffc05286bfc662a9bdf4c", "4bef351d37cdcab0c3b7dfe526b7f0ac0a6063361724711bbc91185c39ab72f8",
          "f1d204e23a2034a1e5b762c15e5727d810f994d2eb0878049460687fd7f3d093"),
}


@pytest.mark.parametrize("name", list(_DIGESTS))
def test_named_nets_keep_their_bits(name):
    n, params, *grads = _DIGESTS[name]
    assert A.n_params(name) == n
    assert hashlib.sha256(A.initial_params(name).tobytes()).hexdigest() == params
    for (seed, norm), want in zip(((0, 50.0), (41, 1.0), (1001, 0.1)), grads):
        assert hashlib.sha256(A.make_gradient(name, seed, norm).tobytes()).hexdigest() == want, (seed, norm)


def test_a_description_is_a_net_of_its_own():
    """A description gives arrays of its own layout and its own draws: the description of net B is not net B's stream."""
    desc = A.NETS["B"]
    assert A.n_params(desc) == A.n_params("B") and A.net_of("B") == A.net_of(desc) == desc
    p, g = A.initial_params(desc), A.make_gradient(desc, 0, 50.0)
    assert p.dtype == g.dtype == np.float32 and p.shape == g.shape == (13529,)
    assert not np.array_equal(p, A.initial_params("B")) and np.array_equal(p, A.initial_params(list(desc)))
    assert abs(float(np.sqrt(np.sum(g.astype(np.float64) ** 2))) - 50.0) < 1e-4
    for i, critic in S.adam_float64_rows([A.NETS[k] for k in "ABC"]):
        d = S.adam_desc(i, critic)
        assert A.n_params(d) == S.n_params(d[:3], critic) == R.param_count(*d[:3], critic)
        assert A.initial_params(d).shape == A.make_gradient(d, 1, 1.0).shape == (A.n_params(d),)


def test_rows_of_the_shape_table_stay_inside_the_budget():
    """The rows tests/test_policy_backward_shapes_gpu.py holds to the float64 step (those that carry a tail n_params % 4 or a boundary
    alignment nets A, B, C do not have), at the step and mode it uses (t = 1, clipping active): the NumPy float32 evaluation alone stays
    inside the committed budgets, which were measured on the three nets and are not raised for these."""
    rows = S.adam_float64_rows([A.NETS[k] for k in "ABC"])
    assert rows == [(0, True), (1, False), (2, False), (7, False)]
    for i, critic in rows:
        desc = S.adam_desc(i, critic)
        p, m, v, g, max_norm, ref = A.one_step_case(desc, 1, "active")
        _, m32, v32, _, info = A.clip_and_adam(p, m, v, 0, g, A.LR, A.BETA1, A.BETA2, A.EPS, max_norm, np.float32)
        dev = A.deviations(m32, v32, info["dp"], ref)
        print(f"{S.row_id(i)} critic {int(critic)} ({A.n_params(desc)} parameters): m {dev[0]:.3f} ulp  v {dev[1]:.3f} ulp  "
              f"|dp32 - dp64| / lr {dev[2]:.3e}")
        assert float(ref[3]["coef"]) < 1.0
        assert dev[0] <= A.BUDGET_M_ULP and dev[1] <= A.BUDGET_V_ULP and dev[2] <= A.BUDGET_P, (i, critic, dev)


def test_tolerances_follow_the_budget():
    p64, m64, v64 = np.array([0.5]), np.array([1.0]), np.array([3.0])
    tp, tm, tv = A.gpu_tolerances(p64, m64, v64)
    assert math.isclose(tp[0], 4 * A.BUDGET_P * A.LR + 0.5 * 2.0 ** -24)
    assert math.isclose(tm[0], max(4 * A.BUDGET_M_ULP, 1.0) * 2.0 ** -23) and math.isclose(tv[0], max(4 * A.BUDGET_V_ULP, 1.0) * 2.0 ** -22)
