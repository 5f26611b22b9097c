"""The recorded rollouts of tests/golden/rollouts (tests/rollout_recordings.py, tools/record_rollouts.py) replayed BIT FOR BIT.

A change that only reorders independent work of a step kernel -- its prologue, its epilogue, the scheduling around the substep
loop -- must leave every output as it was.  The compiler has contracted a sum differently after an unrelated change three times
(quat_unit, reward_total, walk_reward_env), so this is checked, per instantiation, on 40 auto-resetting env-steps with resets on
the way.  If a bit moves: find the expression in the two listings and pin its association in the source; the recordings are
re-made only by a change that means to alter the numbers."""
import numpy as np
import pytest

import rollout_recordings as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(R.FORMS))
def test_rollout_replays_bit_for_bit(name, tmp_path):
    gold = np.load(R.golden_path(name))
    assert (gold["resets"] > 0).any(), "the recording crosses the reset path"
    rec = R.rollout(R.FORMS[name], tmp_path)
    assert set(rec) == set(gold.files)
    moved = []
    for key in gold.files:
        a, b = rec[key], gold[key]
        assert a.shape == b.shape and a.dtype == b.dtype, key
        same = a.view(np.uint8) == b.view(np.uint8) if a.dtype.kind == "f" else a == b
        if not same.all():
            d = np.flatnonzero(~(a == b).reshape(len(a), -1).all(1)) if a.ndim > 1 else np.flatnonzero(a != b)
            moved.append(f"{key}: {len(d)} envs differ (first {d[:4].tolist()}), max |diff| {np.nanmax(np.abs(a.astype(np.float64) - b)):.3g}")
    assert not moved, "; ".join(moved)
