#!/usr/bin/env python3
"""Time the surface-mesh extraction (wo_renderer_mesh_device) pass by pass, and its corner pass
beside the nearest thing the library offered before it: wo_renderer_classify_points_device over a
pre-built float4 buffer of the same corners.

Per scene a grid of --cells^3 cells in the scene's box, --iters bisections.  Timed with HIP events,
`--launches` launches per variant after `--warmup`, the variants alternating in rounds inside one
process (tools/ray_span_bench.py's method).  The variants: the whole extraction into buffers sized
by a counts-only call; the extraction stopped after the corner pass, the count, the scan, the edge
pass (WOLOLO_MESH_PASSES = 1 .. 4; a pass's time is the difference of two neighbours, the vertex
pass's the whole less the first four); the counts-only call; and the point classification of the
corners (up to --baseline-cells cells per axis: its point buffer is 16 bytes per corner).  The
corner bits must equal the point classes with the outer layer cleared.  Needs a GPU; not a test,
not bench.py.

    python tools/mesh_bench.py --out profiles/mesh_bench.txt
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

BOXES = rsb.BOXES  # tests/span_support.py's boxes of these four scenes
PASSES = ("corners", "count", "scan", "edges", "vertices")


def corner_points(grid, h):
    """The corners' float4 rows in corner order, as renderer_ext.h states them (a product and a sum)."""
    f32 = np.float32
    c = [f32(grid.lo[a]) + np.arange(grid.n[a] + 1).astype(f32) * f32(h[a]) for a in range(3)]
    pts = np.zeros((grid.n[2] + 1, grid.n[1] + 1, grid.n[0] + 1, 4), dtype=f32)
    pts[..., 0] = c[0][None, None, :]
    pts[..., 1] = c[1][None, :, None]
    pts[..., 2] = c[2][:, None, None]
    return pts.reshape(-1, 4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", default="256,512", help="cells per axis, a list")
    ap.add_argument("--baseline-cells", type=int, default=256, help="largest grid the point classification is timed on")
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scenes", default=",".join(BOXES))
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_bench: no HIP device (this measurement has no CPU form)")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"mesh_bench: {args.iters} bisections, {args.launches} launches per variant after {args.warmup} in {args.rounds} "
             f"alternating rounds, {torch.cuda.get_device_name(0)}",
             "ms per call; a pass's time is the difference of two runs stopped after neighbouring passes"]
    for scene in args.scenes.split(","):
        r = wl.Renderer(scene, max_nodes=4096)
        scenes.build(scene, r)
        for cells in (int(c) for c in args.cells.split(",")):
            grid = wl.mesh_grid(*BOXES[scene], cells, args.iters)
            h = wl.mesh_grid_check(grid)
            need = wl.mesh_scratch_bytes(grid)
            corners = (cells + 1) ** 3
            d_scratch = torch.zeros(need // 4, dtype=torch.int32, device="cuda")
            d_counts = torch.zeros(4, dtype=torch.int32, device="cuda")
            os.environ.pop("WOLOLO_MESH_PASSES", None)
            r.mesh_device(grid, 0, 0, 0, 0, 0, d_counts.data_ptr(), d_scratch.data_ptr(), need, stream)
            torch.cuda.synchronize()
            nv, nq, caps, _ = (int(x) for x in d_counts.cpu().numpy().view(np.uint32))
            d_v = torch.zeros((max(nv, 1), 4), dtype=torch.int32, device="cuda")
            d_q = torch.zeros((max(nq, 1), 4), dtype=torch.int32, device="cuda")
            d_i = torch.zeros((max(nq, 1), 4), dtype=torch.int32, device="cuda")

            def extract(passes):
                def fn():
                    os.environ["WOLOLO_MESH_PASSES"] = str(passes)
                    r.mesh_device(grid, d_v.data_ptr(), nv, d_q.data_ptr(), d_i.data_ptr(), nq, d_counts.data_ptr(),
                                  d_scratch.data_ptr(), need, stream)
                return fn

            def counts_only():
                os.environ["WOLOLO_MESH_PASSES"] = "5"
                r.mesh_device(grid, 0, 0, 0, 0, 0, d_counts.data_ptr(), d_scratch.data_ptr(), need, stream)

            variants = {("stop", k + 1): extract(k + 1) for k in range(5)}
            variants["counts only"] = counts_only
            baseline = cells <= args.baseline_cells
            if baseline:
                d_pts = torch.from_numpy(corner_points(grid, h)).cuda()
                d_cls = torch.zeros(corners, dtype=torch.int32, device="cuda")
                variants["points"] = lambda: r.classify_points_device(d_pts.data_ptr(), d_cls.data_ptr(), corners, stream)
                # the corner pass computes what the baseline computes: its bits are the classes, outer layer cleared
                variants["points"]()
                extract(1)()
                torch.cuda.synchronize()
                cls = d_cls.cpu().numpy().reshape(cells + 1, cells + 1, cells + 1) == wl.POINT_INSIDE
                cls[[0, -1], :, :] = False
                cls[:, [0, -1], :] = False
                cls[:, :, [0, -1]] = False
                words = (corners + 63) // 64
                bits = np.unpackbits(d_scratch.cpu().numpy().view(np.uint8)[:8 * words], bitorder="little")[:corners]
                if (bits.astype(bool) != cls.reshape(-1)).any():
                    raise RuntimeError(f"{scene} {cells}: the corner bits differ from the point classes")
                del cls, bits
            ms = rsb.time_rounds(variants, args.warmup, args.launches, args.rounds, f"{scene} {cells}^3")
            os.environ.pop("WOLOLO_MESH_PASSES", None)
            whole = ms[("stop", 5)]
            each = [ms[("stop", 1)]] + [ms[("stop", k + 1)] - ms[("stop", k)] for k in range(1, 5)]
            lines.append(f"{scene:13s} {cells}^3 cells, {corners} corners: {nv} vertices, {nq} quads ({caps} caps), scratch "
                         f"{need / 2 ** 20:.0f} MiB;  whole {whole:9.3f} ms ({nq / whole / 1e3:7.2f} Mquads/s), counts only "
                         f"{ms['counts only']:9.3f} ms")
            lines.append(f"{'':13s} " + "   ".join(f"{name} {t:9.3f} ms ({100.0 * t / whole:4.1f} %)" for name, t in zip(PASSES, each)))
            if baseline:
                lines.append(f"{'':13s} corner pass {ms[('stop', 1)]:9.3f} ms ({corners / ms[('stop', 1)] / 1e3:8.1f} Mcorners/s) against "
                             f"classify_points on the same corners {ms['points']:9.3f} ms ({corners / ms['points'] / 1e3:8.1f} "
                             f"Mpoints/s): {ms[('stop', 1)] / ms['points']:5.2f}x")
                del d_pts, d_cls
            del d_scratch, d_v, d_q, d_i
            torch.cuda.empty_cache()
        r.close()
    text = "\n".join(lines + rsb.NOTES) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
