#!/usr/bin/env python3
"""Time the first-hit feature buffers (wo_renderer_render_features_device) at 1920x1080 beside two
baselines from the same build:

  (a) wo_renderer_trace_rays_device on the pre-built batch of the frame's pixel-centre rays, the
      same kernel family -- what a caller could do before, had they the rays;
  (b) the PATHTRACE frame of the same spp through wo_renderer_render_rows_device on the kernel
      AUTO picks -- what the guide layers are added to.

A feature launch traces (spp + 1) rays per pixel, so its time per traced ray is
t / ((spp + 1) pixels); the report sets it against (a)'s time per ray, and the launch against (b).
Both footprints of a wave (WOLOLO_FEATURE_TILE = 8x8 | 64x1) are timed and must give the same
planes.  HIP events, `--launches` launches per variant after `--warmup`, the variants alternating
in `--rounds` rounds inside one process; per variant the median round and the spread (min .. max)
over the rounds.  Needs a GPU; not a test, not bench.py.

    python tools/feature_bench.py --out profiles/feature_bench.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (before libwololo.so: one HIP runtime in the process)

import ray_query_bench as rqb  # noqa: E402
from csgrenderer_amd import scenes  # noqa: E402
from csgrenderer_amd import wololo as wl  # noqa: E402

CASES = [("csg32", "interpreter"), ("csg32_nested", "interpreter"), ("csg256_chain", "interpreter"),
         ("rtiow_cover", "interpreter"), ("rtiow_cover", "lanes")]
SPPS = (1, 8, 64)
TILES = ("8x8", "64x1")
DEFAULT_TILE = "8x8"  # what the library does with no variable set
NOTES = []


def time_rounds(variants, warmup, launches, rounds, what):
    """{name: (median, min, max)} ms per launch over `rounds` rounds of launches / rounds launches
    each between two HIP events, the variants alternating inside every round.  A variant whose host
    enqueue takes more than 0.8 of the measured time gets a note: its figure is an upper bound."""
    per = max(1, launches // rounds)
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    host = {k: 0.0 for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            h0 = time.perf_counter()
            for _ in range(per):
                fn()
            host[name] += (time.perf_counter() - h0) * 1e3
            t1.record()
            torch.cuda.synchronize()
            ms[name].append(t0.elapsed_time(t1) / per)
    for name in variants:
        if host[name] > 0.8 * sum(ms[name]) * per:
            NOTES.append(f"note: {what} {name}: host enqueue {host[name] / (per * rounds):.3f} ms per call against "
                         f"{statistics.median(ms[name]):.3f} ms measured (an upper bound on the kernel's time)")
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--cases", default=",".join(f"{s}:{p}" for s, p in CASES))
    ap.add_argument("--spp", default=",".join(str(s) for s in SPPS))
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("feature_bench: no HIP device (this measurement has no CPU form)")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    w, h = args.width, args.height
    n = w * h
    spps = [int(s) for s in args.spp.split(",")]
    rows = wl.local_rows(h, 16, 1)
    lines = [f"feature_bench: {w}x{h} = {n} pixels, {args.launches} launches per variant after {args.warmup} in "
             f"{args.rounds} alternating rounds, {torch.cuda.get_device_name(0)}",
             "ms per launch: median round (min .. max over the rounds); ns per traced ray = ms / ((spp + 1) pixels);",
             "x(a) = that over (a)'s ns per ray (the bar: 1.15); /frame = the feature launch over (b)"]
    for case in args.cases.split(","):
        scene, path = case.split(":")
        r = wl.Renderer(scene, max_nodes=4096)
        scenes.build(scene, r)
        r.set_ray_tracer(path)
        r.prepare()  # the frame's kernel is the one AUTO settles on
        rays = rqb.pixel_rays(r, wl.render_params(w, h, spp=1, max_depth=1, mode=wl.MODE_NORMALS))
        d_rays = torch.from_numpy(rays.reshape(-1, 8)).cuda()
        d_hits = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        d_planes = torch.zeros((3 * rows * w, 4), dtype=torch.int32, device="cuda")
        d_frame = torch.zeros((rows * w, 4), dtype=torch.float32, device="cuda")

        def first_hit():
            r.trace_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream)

        def features(tile, spp):
            p = wl.render_params(w, h, spp=spp, seed=1, mode=wl.MODE_PATHTRACE)

            def fn():
                os.environ["WOLOLO_FEATURE_TILE"] = tile
                r.render_features_device(p, d_planes.data_ptr(), rows * w, 16, 0, 1, stream)
            return fn

        def frame(spp):
            p = wl.render_params(w, h, spp=spp, seed=1, mode=wl.MODE_PATHTRACE)

            def fn():
                r.render_rows_device(p, d_frame.data_ptr(), 16, 0, 1, stream)
            return fn

        # both footprints give the same planes
        ref = None
        for tile in TILES:
            d_planes.zero_()
            features(tile, spps[0])()
            torch.cuda.synchronize()
            got = d_planes.cpu().numpy().tobytes()
            if ref is None:
                ref = got
            elif got != ref:
                raise RuntimeError(f"{scene} {path}: footprint {tile} gives other planes than {TILES[0]}")
        kernel_path = r.ray_path()
        variants = {("rays",): first_hit}
        for spp in spps:
            for tile in TILES:
                variants[(tile, spp)] = features(tile, spp)
            variants[("frame", spp)] = frame(spp)
        ms = time_rounds(variants, args.warmup, args.launches, args.rounds, f"{scene} {path}")
        a, a_lo, a_hi = ms[("rays",)]
        lines.append(f"{scene:13s} {kernel_path:11s} (a) trace_rays on the pixel rays {a:8.3f} ms ({a_lo:.3f} .. {a_hi:.3f}), "
                     f"{a * 1e6 / n:6.3f} ns per ray;  frames on \"{r.trace_path()}\"")
        for spp in spps:
            b, b_lo, b_hi = ms[("frame", spp)]
            lines.append(f"{'':13s} spp {spp:2d}: (b) frame {b:9.3f} ms ({b_lo:.3f} .. {b_hi:.3f})")
            for tile in TILES:
                t, lo, hi = ms[(tile, spp)]
                per_ray = t * 1e6 / ((spp + 1) * n)
                mark = "  <- default" if tile == DEFAULT_TILE else ""
                lines.append(f"{'':13s}         features {tile:4s} {t:9.3f} ms ({lo:.3f} .. {hi:.3f}), {per_ray:6.3f} ns per ray, "
                             f"{per_ray / (a * 1e6 / n):5.2f} x(a), {t / b:5.2f} /frame{mark}")
        os.environ.pop("WOLOLO_FEATURE_TILE", None)
        r.close()
        print(f"feature_bench: {scene} {path} done", flush=True)
    text = "\n".join(lines + NOTES) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
