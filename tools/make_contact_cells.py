"""Generate tests/golden/contact_cells.npz: f32 states (qpos, qvel, act, nstep, actions) that put every ground-contact sample point
of the robot on the floor, grazing and pressed, plus the cull-edge states, with the cell each state belongs to (kind, body, point,
depth_class).  No oracle outputs: the tests recompute them.  The generator and the census live in tests/contact_cells.py; like
tools/make_golden.py this only runs them and writes the file.  Run:  python tools/make_contact_cells.py [-v]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contact_cells as CC  # noqa: E402
from oracle import oracle as O  # noqa: E402
from parity import TOL  # noqa: E402


def main():
    fix = CC.generate(O, TOL["A"], log=print if "-v" in sys.argv else None)
    np.savez_compressed(CC.FIXTURE, **fix)
    cen = CC.census(O, O.default_model(), fix, labels=fix)
    print("wrote", CC.FIXTURE, os.path.getsize(CC.FIXTURE), "bytes;", len(fix["qpos"]), "states")
    print("points never touched:", cen["untouched"], "of", int(cen["valid"].sum()))
    print("points with a state in which they are alone on their body:", int((cen["alone"].any(0) & cen["valid"]).sum()))
    print("deepest state: %.2f mm; cells above 6 mm: %d" % (1e3 * cen["deepest"].max(), len(cen["deep_cells"])))
    for b, i, d, depth in cen["deep_cells"]:
        print("   %s: %.1f mm" % (CC.cell_name(b, i, d), 1e3 * depth))
    print("states per body and branch (%s):" % ", ".join(CC.BRANCHES))
    print(cen["branch"].sum(0))
    per_cell, one, two = CC.shift_coverage(O, fix, TOL["A"])
    for d in (CC.GRAZE, CC.PRESS):
        n = sum(bool((v > CC.MARGIN).all()) for k, v in per_cell.items() if k[2] == d)
        print("%s cells that clear all six 1 mm shifts by themselves: %d of 108" % (CC.DEPTH_NAMES[d], n))
    print("points that need the 2 mm shift: %d" % len(two))
    for (b, i), ex in two.items():
        print("   body %d point %d: 1 mm %s, 2 mm %s" % (b, i, np.round(one[(b, i)], 2), np.round(ex, 2)))


if __name__ == "__main__":
    main()
