"""Generate tests/golden/quadruped_model/: the reference robot's two MJCF files and, per OBJ mesh, its vertex positions.

The compiler (quadruped-gym_amd/model/compiler.py, mesh_inertia="convex") reads nothing of a mesh but its vertex positions: mass
properties come from their convex hull, contact points are picked among the hull's vertices.  The hull is built incrementally, so
its triangulation -- and with it the last bit of the mass properties -- depends on every vertex and its order: all of them are kept,
in order, with their text as written, and the rest of each OBJ (colours, faces) is dropped.  xz compression takes the 2.9 MB of
meshes to ~50 kB.  tests/helpers.py:reference_model() unpacks the fixture into a temporary directory.
Run:  python tools/make_model_fixture.py <reference>/src/models/quadruped
"""
import lzma
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "quadruped_model")


def main(src):
    os.makedirs(os.path.join(OUT, "mesh"), exist_ok=True)
    for name in ("scene.xml", "quadruped.xml"):
        shutil.copyfile(os.path.join(src, name), os.path.join(OUT, name))
    for name in sorted(os.listdir(os.path.join(src, "mesh"))):
        if not name.endswith(".obj"):
            continue
        with open(os.path.join(src, "mesh", name)) as fh:
            verts = [" ".join(line.split()[:4]) for line in fh if line.startswith("v ")]
        text = f"# vertex positions of {name} (faces and colours dropped: the convex-hull compile does not read them)\n"
        text += "\n".join(verts) + "\n"
        with lzma.open(os.path.join(OUT, "mesh", name + ".xz"), "wb", preset=9) as fh:
            fh.write(text.encode())
        print(name, len(verts), "vertices")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
