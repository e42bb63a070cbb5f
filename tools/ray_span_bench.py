#!/usr/bin/env python3
"""Time ray span queries (wo_renderer_trace_spans_device) and point classification
(wo_renderer_classify_points_device) beside the first-hit query on the same rays.

Per scene a width x height batch: the pixel rays of csg32 and csg32_nested, and an equally large
grid of parallel rays through csg256_chain and rtiow_cover (origins on a plane 1.0 outside the
scene's box, direction +x).  Timed with HIP events, `--launches` launches per variant after
`--warmup`, the variants alternating in rounds inside one process: wo_renderer_trace_rays_device
with the interpreter (the first-hit query), and trace_spans at max_crossings 0, 8 and 32 for each
sweep window (WOLOLO_SPAN_WINDOW = 4, 8, 16).  Then classify_points on `--points` points uniform
in each scene's box.  Needs a GPU; not a test, not bench.py.

    python tools/ray_span_bench.py --out profiles/ray_span_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (before libwololo.so: one HIP runtime in the process)

from csgrenderer_amd import scenes  # noqa: E402
from csgrenderer_amd import wololo as wl  # noqa: E402
from ray_query_bench import pixel_rays  # noqa: E402

BOXES = {
    "csg32": ((-6.5, -1.0, -6.5), (6.5, 3.0, 6.5)),
    "csg32_nested": ((-3.0, -1.2, -3.0), (3.0, 4.4, 3.0)),
    "csg256_chain": ((-5.0, -0.5, -5.0), (5.0, 3.0, 5.0)),
    "rtiow_cover": ((-11.0, -0.5, -11.0), (11.0, 2.5, 11.0)),
}
BATCH = {"csg32": "pixel rays", "csg32_nested": "pixel rays", "csg256_chain": "through rays",
         "rtiow_cover": "through rays"}
WINDOWS = (4, 8, 16)
MAX_CROSSINGS = (0, 8, 32)


def through_grid(box, w, h):
    """w x h parallel rays along +x from the plane 1.0 outside the box: z over the width, y over
    the height (pixel-centre spacing), consecutive rays neighbours in z."""
    lo, hi = (np.array(b, dtype=np.float64) for b in box)
    z = lo[2] + (np.arange(w) + 0.5) * (hi[2] - lo[2]) / w
    y = hi[1] - (np.arange(h) + 0.5) * (hi[1] - lo[1]) / h
    rays = np.zeros((h, w, 8), dtype=np.float32)
    rays[..., 0] = lo[0] - 1.0
    rays[..., 1] = y[:, None]
    rays[..., 2] = z[None, :]
    rays[..., 3] = np.inf
    rays[..., 4] = 1.0
    return rays.reshape(-1, 8)


def time_rounds(variants, warmup, launches, rounds, what):
    """ms per launch of every variant {name: fn}, the variants alternating: `rounds` rounds, in
    each `launches / rounds` launches of each variant between two HIP events.  The host must
    enqueue faster than the device runs for that to be the kernel's time: a variant whose
    enqueue time per call exceeds 0.8 of the measured time gets a note (`what` names it)."""
    per = max(1, launches // rounds)
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    total = {k: 0.0 for k in variants}
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
            total[name] += t0.elapsed_time(t1)
    for name in variants:
        if host[name] > 0.8 * total[name]:
            NOTES.append(f"note: {what} {name}: host enqueue {host[name] / (per * rounds):.3f} ms per call against "
                         f"{total[name] / (per * rounds):.3f} ms measured (an upper bound on the kernel's time)")
    return {k: v / (per * rounds) for k, v in total.items()}


NOTES = []


def set_window(w):
    os.environ["WOLOLO_SPAN_WINDOW"] = str(w)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--points", type=int, default=1 << 21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--scenes", default=",".join(BOXES))
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ray_span_bench: no HIP device (this measurement has no CPU form)")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    n = args.width * args.height
    lines = [f"ray_span_bench: {args.width}x{args.height} = {n} rays, {args.points} points, {args.launches} launches "
             f"per variant after {args.warmup} in {args.rounds} alternating rounds, {torch.cuda.get_device_name(0)}",
             "ms per launch (Mrays/s; spans / first-hit) by sweep window"]
    for scene in args.scenes.split(","):
        r = wl.Renderer(scene, max_nodes=4096)
        scenes.build(scene, r)
        if BATCH[scene] == "pixel rays":
            rays = pixel_rays(r, wl.render_params(args.width, args.height, spp=1, max_depth=1, mode=wl.MODE_NORMALS))
        else:
            rays = through_grid(BOXES[scene], args.width, args.height)
        d_rays = torch.from_numpy(rays).cuda()
        d_hits = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
        d_spans = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
        d_cross = torch.zeros((max(MAX_CROSSINGS), n, 16), dtype=torch.uint8, device="cuda")
        r.set_ray_tracer("interpreter")

        def first_hit():
            r.trace_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream)

        def spans(window, maxc):
            def fn():
                set_window(window)
                r.trace_spans_device(d_rays.data_ptr(), d_spans.data_ptr(), d_cross.data_ptr() if maxc else 0, n, maxc,
                                     stream)
            return fn

        # the windows agree with each other, and crossing 0 with the first-hit query
        first_hit()
        torch.cuda.synchronize()
        hits = d_hits.cpu().numpy().reshape(-1).view(np.dtype(wl.RAY_HIT_FIELDS))
        ref = None
        for w in WINDOWS:
            spans(w, 8)()
            torch.cuda.synchronize()
            got = (d_spans.cpu().numpy().tobytes(), d_cross[:1].cpu().numpy().tobytes())
            if ref is None:
                ref = got
                summary = d_spans.cpu().numpy().reshape(-1).view(np.dtype(wl.RAY_SPANS_FIELDS)).copy()
                c0 = d_cross[0].cpu().numpy().reshape(-1).view(np.dtype(wl.RAY_CROSSING_FIELDS))
                hit = (hits["flags"] & wl.RAY_HIT) != 0
                if not ((summary["count"] > 0) == hit).all() or c0["t"][hit].tobytes() != hits["t"][hit].tobytes():
                    raise RuntimeError(f"{scene}: crossing 0 differs from the first-hit query")
            elif got != ref:
                raise RuntimeError(f"{scene}: window {w} gives other spans than window {WINDOWS[0]}")
        variants = {"first-hit": first_hit}
        for w in WINDOWS:
            for m in MAX_CROSSINGS:
                variants[(w, m)] = spans(w, m)
        ms = time_rounds(variants, args.warmup, args.launches, args.rounds, scene)
        base = ms["first-hit"]
        cnt = summary["count"]
        lines.append(f"{scene:13s} {BATCH[scene]:12s} crossings per ray: mean {cnt.mean():.2f}, max {cnt.max()}, "
                     f"{(cnt > 0).mean():.3f} hit;  first-hit (interpreter) {base:8.3f} ms ({n / base / 1e3:8.1f} Mrays/s)")
        for m in MAX_CROSSINGS:
            cols = "   ".join(f"w{w:<2d} {ms[(w, m)]:8.3f} ms ({n / ms[(w, m)] / 1e3:8.1f}; {ms[(w, m)] / base:5.2f}x)"
                              for w in WINDOWS)
            lines.append(f"{'':13s} spans max_crossings {m:2d}:  {cols}")
        del d_cross, d_hits
        os.environ.pop("WOLOLO_SPAN_WINDOW", None)
        # points uniform in the scene's box
        lo, hi = (np.array(b) for b in BOXES[scene])
        pts = np.zeros((args.points, 4), dtype=np.float32)
        pts[:, :3] = np.random.default_rng(3).uniform(lo, hi, size=(args.points, 3))
        d_pts = torch.from_numpy(pts).cuda()
        d_in = torch.zeros(args.points, dtype=torch.int32, device="cuda")
        pms = time_rounds({"points": lambda: r.classify_points_device(d_pts.data_ptr(), d_in.data_ptr(), args.points,
                                                                      stream)},
                          args.warmup, args.launches, args.rounds, scene)["points"]
        inside = float((d_in.cpu().numpy() == wl.POINT_INSIDE).mean())
        lines.append(f"{'':13s} classify_points: {pms:8.3f} ms ({args.points / pms / 1e3:8.1f} Mpoints/s, "
                     f"{inside:.3f} inside)")
        r.close()
    text = "\n".join(lines + NOTES) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
