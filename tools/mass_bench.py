#!/usr/bin/env python3
"""Time the mass-properties query (wo_renderer_mass_sums_device) beside the nearest thing the
library offered before it: the thickness query (wo_renderer_trace_spans_device with
max_crossings = 0) on a pre-built ray grid of the same cells.

Per scene a width x height grid of cells in the scene's box, rays along --axis.  Timed with HIP
events, `--launches` launches per variant after `--warmup`, the variants alternating in rounds
inside one process (tools/ray_span_bench.py's method): the thickness query at sweep windows 8 and
16, and the mass kernel in every form -- a wave's footprint 8x8 or 64x1 cells (WOLOLO_MASS_TILE),
the window 8 or 16 (WOLOLO_MASS_WINDOW), the accumulators in registers, reduced across the wave per
ray, or in LDS slots (WOLOLO_MASS_REDUCE = regs | shfl | lds); and, for the register forms at
window 16, the final atomic adds issued per wave instead of per workgroup (WOLOLO_MASS_FLUSH = wave).
All forms must give the same Wo_MassSums.  Needs a GPU; not a test, not bench.py.

    python tools/mass_bench.py --out profiles/mass_bench.txt
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
TILES = ("8x8", "64x1")
WINDOWS = (8, 16)
REDUCES = ("regs", "shfl", "lds")
DEFAULT = ("8x8", 16, "regs")  # what the library does with no variable set


def grid_rays(grid, plan):
    """The grid's Wo_Ray rows as renderer_ext.h states them (float32, a product and a sum), row-major."""
    axis, u, v = grid.axis, (grid.axis + 1) % 3, (grid.axis + 2) % 3
    f32 = np.float32
    cu = f32(plan.u0) + (2 * np.arange(grid.nu) + 1).astype(f32) * f32(plan.hu)
    cv = f32(plan.v0) + (2 * np.arange(grid.nv) + 1).astype(f32) * f32(plan.hv)
    rays = np.zeros((grid.nv, grid.nu, 8), dtype=f32)
    rays[..., axis] = plan.o_axis
    rays[..., u] = cu[None, :]
    rays[..., v] = cv[:, None]
    rays[..., 3] = plan.t_max
    rays[..., 4 + axis] = 1.0
    return rays.reshape(-1, 8)


def set_form(tile, window, reduce, flush="block"):
    os.environ["WOLOLO_MASS_FLUSH"] = flush
    os.environ["WOLOLO_MASS_TILE"] = tile
    os.environ["WOLOLO_MASS_WINDOW"] = str(window)
    os.environ["WOLOLO_MASS_REDUCE"] = reduce


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--axis", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--scenes", default=",".join(BOXES))
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mass_bench: no HIP device (this measurement has no CPU form)")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    n = args.width * args.height
    lines = [f"mass_bench: {args.width}x{args.height} = {n} cells, rays along axis {args.axis}, {args.launches} launches per "
             f"variant after {args.warmup} in {args.rounds} alternating rounds, {torch.cuda.get_device_name(0)}",
             "ms per launch (ratio to the thickness query at the same sweep window)"]
    for scene in args.scenes.split(","):
        r = wl.Renderer(scene, max_nodes=4096)
        scenes.build(scene, r)
        grid = wl.mass_grid(*BOXES[scene], args.axis, args.width, args.height)
        plan = wl.mass_grid_plan(grid)
        d_rays = torch.from_numpy(grid_rays(grid, plan)).cuda()
        d_spans = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
        d_sums = torch.zeros(24, dtype=torch.int64, device="cuda")

        def thickness(window):
            def fn():
                os.environ["WOLOLO_SPAN_WINDOW"] = str(window)
                r.trace_spans_device(d_rays.data_ptr(), d_spans.data_ptr(), 0, n, 0, stream)
            return fn

        def mass(tile, window, reduce, flush="block"):
            def fn():  # (timed launches keep adding into d_sums; the integers wrap, the time does not care)
                set_form(tile, window, reduce, flush)
                r.mass_sums_device(grid, d_sums.data_ptr(), stream)
            return fn

        # every form gives the same sums, and their crossings are the thickness query's
        thickness(16)()
        torch.cuda.synchronize()
        spans = d_spans.cpu().numpy().reshape(-1).view(np.dtype(wl.RAY_SPANS_FIELDS))
        ref = None
        for tile in TILES:
            for window in WINDOWS:
                for reduce in REDUCES:
                    for flush in ("block", "wave"):
                        d_sums.zero_()
                        mass(tile, window, reduce, flush)()
                        torch.cuda.synchronize()
                        got = d_sums.cpu().numpy().tobytes()
                        if ref is None:
                            ref = got
                        elif got != ref:
                            raise RuntimeError(f"{scene}: form {tile} w{window} {reduce} {flush} gives other sums")
        sums = wl.MassSums.from_buffer_copy(ref)
        if sums.rays != n or sums.crossings != int(spans["count"].sum(dtype=np.uint64)):
            raise RuntimeError(f"{scene}: the mass query's rays or crossings differ from the thickness query's")
        props = wl.mass_properties_from_sums(grid, sums)
        variants = {("thickness", w): thickness(w) for w in WINDOWS}
        for tile in TILES:
            for window in WINDOWS:
                for reduce in REDUCES:
                    variants[(tile, window, reduce)] = mass(tile, window, reduce)
            variants[(tile, "wave flush")] = mass(tile, 16, "regs", "wave")
        ms = rsb.time_rounds(variants, args.warmup, args.launches, args.rounds, scene)
        lines.append(f"{scene:13s} crossings per ray: mean {sums.crossings / n:.2f}, {sums.rays_hit / n:.3f} hit, volume "
                     f"{props.volume:.6g};  thickness query w8 {ms[('thickness', 8)]:7.3f} ms, w16 {ms[('thickness', 16)]:7.3f} ms")
        for tile in TILES:
            for reduce in REDUCES:
                cols = "   ".join(f"w{w:<2d} {ms[(tile, w, reduce)]:7.3f} ms ({ms[(tile, w, reduce)] / ms[('thickness', w)]:5.2f}x)"
                                  for w in WINDOWS)
                mark = "  <- default at w%d" % DEFAULT[1] if (tile, reduce) == (DEFAULT[0], DEFAULT[2]) else ""
                lines.append(f"{'':13s} mass {tile:4s} {reduce:4s}:  {cols}{mark}")
        lines.append(f"{'':13s} mass regs w16, atomic adds per wave instead of per workgroup:  "
                     + "   ".join(f"{tile} {ms[(tile, 'wave flush')]:7.3f} ms" for tile in TILES))
        for k in ("WOLOLO_MASS_FLUSH", "WOLOLO_MASS_TILE", "WOLOLO_MASS_WINDOW", "WOLOLO_MASS_REDUCE", "WOLOLO_SPAN_WINDOW"):
            os.environ.pop(k, None)
        r.close()
    text = "\n".join(lines + rsb.NOTES) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
