#!/usr/bin/env python3
"""Write the closed quad mesh of a scenes.py scene as a Wavefront OBJ file: wo_renderer_mesh on a
grid of --cells^3 cells over the scene's box (tests/span_support.py's, or --box), then
wo_mesh_write_obj with the faces grouped by node.  The file is read back and its directed-edge
balance checked (every edge p->q of the quads occurs as often as q->p).  Needs a GPU.

    python tools/mesh_export.py --scene csg32 --cells 128 out.obj
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (before libwololo.so: one HIP runtime in the process)

import ray_span_bench as rsb  # noqa: E402
from csgrenderer_amd import scenes  # noqa: E402
from csgrenderer_amd import wololo as wl  # noqa: E402


def read_faces(path):
    """(number of v lines, faces (m, 4) 0-based) of an OBJ file of quads."""
    nv, faces = 0, []
    with open(path) as fh:
        for line in fh:
            if line.startswith("v "):
                nv += 1
            elif line.startswith("f "):
                faces.append([int(x) - 1 for x in line.split()[1:5]])
    return nv, np.array(faces, dtype=np.int64).reshape(-1, 4)


def unbalanced_edges(quads):
    """0 iff every directed edge occurs as often as its reverse (else how many sorted keys differ)."""
    a, b = quads.reshape(-1), np.roll(quads, -1, axis=1).reshape(-1)
    big = int(quads.max()) + 1 if len(quads) else 1
    return int((np.sort(a * big + b) != np.sort(b * big + a)).sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="csg32")
    ap.add_argument("--cells", type=int, default=128)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--box", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_export: no HIP device")
    if args.box is None and args.scene not in rsb.BOXES:
        sys.exit(f"mesh_export: no box is known for {args.scene}; give --box")
    lo, hi = (args.box[:3], args.box[3:]) if args.box else rsb.BOXES[args.scene]
    torch.cuda.set_device(0)
    r = wl.Renderer(args.scene, max_nodes=4096)
    scenes.build(args.scene, r)
    vertices, quads, ids, counts = r.mesh(wl.mesh_grid(lo, hi, args.cells, args.iters))
    r.close()
    wl.write_obj(args.out, vertices, quads, ids)
    nv, faces = read_faces(args.out)
    bad = unbalanced_edges(faces)
    print(f"mesh_export: {args.scene} at {args.cells}^3 cells: {counts.vertices} vertices, {counts.quads} quads "
          f"({counts.cap_quads} caps) -> {args.out}; read back {nv} vertices, {len(faces)} faces, {bad} unbalanced edges")
    if nv != counts.vertices or len(faces) != counts.quads or bad:
        sys.exit("mesh_export: the file does not parse back to the balanced mesh")


if __name__ == "__main__":
    main()
