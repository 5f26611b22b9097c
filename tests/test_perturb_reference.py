"""The perturbation layer's checker (tests/perturb_reference.py) without a GPU: its integers are the oracle's hash, its normals have the
moments of a standard normal on the samples the GPU test reuses, its delays are uniform, and the error budget E_z of a float32
evaluation is measured (with QG_PERTURB_PARITY_OUT=<file> the figures are appended to that file: profiles/r24/perturb_parity.txt).

Checked here in float64: the worst |mean| / lag-1 correlation / |std - 1| of the nine observation samples are 0.011 / 0.020 / 0.007
against 0.0245 / 0.0245 / 0.0173."""
import os

import numpy as np

import perturb_reference as R


def _report(line):
    path = os.environ.get("QG_PERTURB_PARITY_OUT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def test_integers_are_the_oracles_hash(oracle):
    L = oracle.lib()
    rng = np.random.default_rng(7)
    cases = [(0, 0, 0, 0), (1, 3, 2, 4096), (12345, 66, 7, R.frame_stream(63, 25)), (2 ** 64 - 1, 2 ** 40, 2 ** 33, 2 ** 31 + 5)]
    cases += [tuple(int(v) for v in rng.integers(0, 2 ** 31, 4)) for _ in range(200)]
    for seed, env, ep, stream in cases:
        stream = int(stream)
        assert int(R.k_int(seed, env, ep, stream, salted=False)[0]) == L.qgo_uniform_stream(seed, env, ep, stream) * 2.0 ** 24
        assert int(R.k_int(seed, env, ep, stream)[0]) == L.qgo_uniform_stream((seed + R.SALT) % 2 ** 64, env, ep, stream) * 2.0 ** 24
    # vectorised and one at a time agree
    e, s = np.ix_(np.arange(5), np.arange(4096, 4106))
    assert np.array_equal(R.k_int(3, e, 2, s), [[int(R.k_int(3, i, 2, j)[0]) for j in range(4096, 4106)] for i in range(5)])


def test_streams_do_not_overlap():
    """z(s) reads k(s) and k(s + 1): the delay (0, unpaired), the biases 2 + 2c .. 129 and the frame draws from 4096 on, each pair of
    its own."""
    bias = R.bias_stream(np.arange(64))
    frame = R.frame_stream(*np.ix_(np.arange(3), np.arange(64 + R.NJ))).ravel()
    used = np.concatenate([[0], bias, bias + 1, frame, frame + 1])
    assert len(set(used.tolist())) == used.size and bias.max() + 1 < 4096
    assert R.frame_stream(1, 0) - R.frame_stream(0, 64 + R.NJ - 1) >= 2


def test_normals_have_standard_moments():
    assert abs(R.z64(0, np.arange(1000), 0, 4096)).max() <= np.sqrt(48 * np.log(2))
    worst = np.zeros(3)
    for seed in R.MOMENT_SEEDS:
        for ep in R.MOMENT_EPISODES:
            for name, sample in (("obs", R.obs_sample), ("action", R.action_sample), ("bias", R.bias_sample)):
                got = R.assert_moments(sample(seed, ep), (name, seed, ep))
                _report(f"checker f64 {name:6s} seed {seed:5d} episode {ep}: |mean| {got[0]:.4f} |std-1| {got[1]:.4f} lag-1 {got[2]:.4f}")
                if name == "obs":
                    worst = np.maximum(worst, got)
    n = R.MOMENT_ENVS * R.MOMENT_FRAMES * R.MOMENT_COLS
    assert abs(4 / np.sqrt(n) - 0.0245) < 1e-4 and abs(4 / np.sqrt(2 * n) - 0.0173) < 1e-4
    # the float32 evaluation passes too (what the kernel computes is such an evaluation)
    R.assert_moments(R.obs_sample(12345, 7, R.z32), "f32")


def test_delays_are_uniform():
    lo, hi = R.DELAY_RANGE
    sigma = np.sqrt(R.DELAY_ENVS * 0.25 * 0.75)
    for seed in R.MOMENT_SEEDS:
        for ep in R.MOMENT_EPISODES:
            d = R.delay_of(seed, np.arange(R.DELAY_ENVS), ep, lo, hi)
            counts = np.bincount(d, minlength=4)
            assert counts.size == 4 and d.min() >= lo and d.max() <= hi
            _report(f"checker delays seed {seed:5d} episode {ep}: counts {counts.tolist()}")
            assert np.all(np.abs(counts - R.DELAY_ENVS / 4) <= 4 * sigma), (seed, ep, counts)
    assert np.all(R.delay_of(5, np.arange(100), 3, 2, 2) == 2)


def test_error_budget_is_measured():
    """E_z is taken from a float32 evaluation of the definition, not from the kernel.  It has to be a float32-sized number: the
    argument 2 pi u2 < 6.3 is rounded to 2^-22 at most, the constant by 1.8e-7 of it, and |z| < 5.77 carries a few ulps of 4.8e-7."""
    ez = R.error_budget()
    _report(f"E_z (float32 NumPy evaluation of z against float64, {len(R.MOMENT_SEEDS) * len(R.MOMENT_EPISODES)} x 3 samples): {ez:.3e}")
    assert 1e-7 < ez < 1e-5


def test_checker_keeps_a_frames_noise_through_the_stack():
    """The property the definitions exist for, on the checker itself: within an episode slot k of step t equals slot k + 1 of step
    t - 1; a finished env's row belongs to the right episode."""
    n, W, F = 10, 3, 4
    obs_std, bias_std = R.column_stds(F)
    ck = R.Checker(n, F, W, obs_std=obs_std, bias_std=bias_std, done_row="reset", seed=3)
    done = R.done_table(n)
    prev, zeros = None, np.zeros((n, W * F))
    for t in range(R.STEPS):
        out = ck.observe(zeros, done[t], terminal=zeros)
        row = out["ref"].reshape(n, W, F)
        if prev is not None:
            live = ~done[t].astype(bool)
            assert np.array_equal(row[live, :-1], prev[live, 1:])
        fin = done[t].astype(bool)
        assert np.all(out["top"][fin] == 0) and np.all(row[fin] == row[fin][:, :1])        # frame 0 of the new episode in every slot
        if prev is not None and fin.any():
            assert np.array_equal(out["term_ref"].reshape(n, W, F)[fin, :-1], prev[fin, 1:])      # the old episode's frames
        prev = row
    assert ck.episode.tolist() == [0, 1, 1, 1, 3] * 2
