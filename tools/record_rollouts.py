"""Record the seeded rollouts of tests/rollout_recordings.py with the CURRENT build: tests/golden/rollouts/<form>.npz.

Run it on the GPU with the build whose bits are to be kept (before a change that must not move them); tests/test_rollout_bits_gpu.py
then replays every recording against whatever is built.  usage: record_rollouts.py [out_dir] [form ...]"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rollout_recordings as R  # noqa: E402


def main():
    args = sys.argv[1:]
    out_dir = args.pop(0) if args and args[0] not in R.FORMS else R.GOLDEN
    os.makedirs(out_dir, exist_ok=True)
    none = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in (args or R.FORMS):
            rec = R.rollout(R.FORMS[name], tmp)
            np.savez_compressed(os.path.join(out_dir, name + ".npz"), **rec)
            nreset = int((rec["resets"] > 0).sum())
            print(f"{name:14s} {R.FORMS[name].kernel:38s} envs reset: {nreset:3d}  resets: {int(rec['resets'].sum()):3d}", flush=True)
            if nreset == 0:
                none.append(name)
    assert not none, f"no env was reset in {none}: the recording does not cross the reset path"


if __name__ == "__main__":
    main()
