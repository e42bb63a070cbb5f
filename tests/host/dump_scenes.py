"""Scene dumps for the lane BVH builder's stand-alone driver (lane_bvh_main.cpp):
python tests/host/dump_scenes.py OUT_DIR [scene ...] writes OUT_DIR/<scene>.bin
(u32 n_recs, n_prims, n_mats; the records; the materials).  No GPU needed."""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
os.environ.setdefault("WOLOLO_ALLOW_NO_DEVICE", "1")

from csgrenderer_amd import scenes, wololo as wl  # noqa: E402

DEFAULT = ("csg32_union", "rtiow_cover", "csg32", "csg256_balanced", "csg512_balanced", "csg32_nested", "csg256_chain",
           "csg360_nested")

if __name__ == "__main__":
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    for name in sys.argv[2:] or DEFAULT:
        r = wl.Renderer(name, max_nodes=4096)
        scenes.build(name, r)
        prog, n_recs, n_prims = r.program()
        mats, n_mats = r.materials()
        with open(os.path.join(out, name + ".bin"), "wb") as f:
            f.write(struct.pack("<3I", n_recs, n_prims, n_mats))
            f.write(bytes(prog)[:32 * n_recs])
            f.write(bytes(mats)[:32 * n_mats])
        r.close()
