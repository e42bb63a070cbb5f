#!/usr/bin/env python3
"""Time ray queries (wo_renderer_trace_rays_device) against the NORMALS frame of the same
size on the matching path kernel.

Per scene (csg32, rtiow_cover) and per ray kernel that applies (interpreter; lanes on
union-only scenes): the width x height batch of pixel rays, HIP events around `--launches`
launches after `--warmup`; beside it wo_renderer_render_rows_device of the WO_SHADING_NORMALS
frame with set_tracer(interpreter | lanes) -- the same rays, 16 B written per pixel where the
query reads 32 B and writes 32 B per ray.  Then the incoherent case on rtiow_cover: as many
rays with origins uniform in the scene's box and uniform directions, interpreter against
lanes.  Needs a GPU; not a test, not bench.py.

    python tools/ray_query_bench.py --out profiles/ray_query_bench.txt
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libwololo.so: one HIP runtime in the process)

from csgrenderer_amd import scenes  # noqa: E402
from csgrenderer_amd import wololo as wl  # noqa: E402

FORMS = {"csg32": ("interpreter",), "rtiow_cover": ("interpreter", "lanes")}
INCOHERENT_BOX = ((-11.0, -0.5, -11.0), (11.0, 2.5, 11.0))  # rtiow_cover


def pixel_rays(r, p):
    """wo_renderer_pixel_ray for every pixel of the frame, restated in float32 numpy (one
    rounding per operation, as the C) and checked against the library on sampled pixels."""
    f32 = np.float32
    cam = r.frame_desc(p).cam
    v3 = lambda a: np.array(list(a), dtype=f32)  # noqa: E731
    origin, ll, hz, vt = v3(cam.origin), v3(cam.lower_left), v3(cam.horizontal), v3(cam.vertical)
    w, h = p.width, p.height
    u = (np.arange(w, dtype=f32) + f32(0.5)) * (f32(1.0) / f32(w))
    v = (f32(h - 1) - np.arange(h, dtype=f32) + f32(0.5)) * (f32(1.0) / f32(h))
    d = ((ll[None, None, :] + u[None, :, None] * hz[None, None, :]) + v[:, None, None] * vt[None, None, :]) - origin
    d = d - f32(0.0)
    dot = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    inv = f32(1.0) / np.sqrt(np.maximum(dot, f32(2.0 ** -96)))
    d = d * inv[..., None]
    rays = np.zeros((h, w, 8), dtype=f32)
    rays[..., 0:3] = origin + f32(0.0)
    rays[..., 3] = np.inf
    rays[..., 4:7] = d
    rng = np.random.default_rng(1)
    for x, y in zip(rng.integers(0, w, 64), rng.integers(0, h, 64)):
        if rays[y, x].tobytes() != r.pixel_ray(p, x, y).tobytes():
            raise RuntimeError(f"pixel_rays: pixel ({x}, {y}) differs from wo_renderer_pixel_ray")
    return rays.reshape(-1, 8)


def incoherent_rays(n, box, seed=5):
    rng = np.random.default_rng(seed)
    lo, hi = (np.array(b) for b in box)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.sqrt((d * d).sum(axis=1, dtype=np.float32), dtype=np.float32)[:, None]
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, 0:3] = rng.uniform(lo, hi, size=(n, 3))
    rays[:, 3] = np.inf
    rays[:, 4:7] = d
    return rays


def time_ms(fn, warmup, launches):
    """ms per call of fn() on the current stream (HIP events around `launches` calls).  The
    host must enqueue faster than the device runs for that to be the kernel's time: the
    enqueue time per call is returned beside it: (device ms, host enqueue ms)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    h0 = time.perf_counter()
    for _ in range(launches):
        fn()
    h1 = time.perf_counter()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / launches, (h1 - h0) * 1e3 / launches


NOTES = []


def _bound(timing, what):
    """The device time of a (device ms, host enqueue ms) pair; a note when the host's enqueue
    rate, not the kernel, may have set it."""
    ms, host_ms = timing
    if host_ms > 0.8 * ms:
        NOTES.append(f"note: {what}: host enqueue {host_ms:.3f} ms per call against {ms:.3f} ms measured "
                     f"(an upper bound on the kernel's time)")
    return ms


def time_query(r, rays, form, warmup, launches):
    stream = torch.cuda.current_stream().cuda_stream
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.zeros((len(rays), 32), dtype=torch.uint8, device="cuda")
    r.set_ray_tracer(form)
    ms = time_ms(lambda: r.trace_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), len(rays), stream), warmup,
                 launches)
    ms = _bound(ms, f"{form} query")
    if r.ray_path() != form:
        raise RuntimeError(f"asked for the {form} ray kernel, ran {r.ray_path()}")
    hits = d_hits.cpu().numpy().reshape(-1).view(np.dtype(wl.RAY_HIT_FIELDS))
    return ms, float(((hits["flags"] & wl.RAY_HIT) != 0).mean()), hits


def time_normals(r, p, form, warmup, launches):
    stream = torch.cuda.current_stream().cuda_stream
    r.set_tracer(form)
    rows = wl.local_rows(p.height, 4, 1)
    d_out = torch.zeros((rows, p.width, 4), dtype=torch.float32, device="cuda")
    ms = _bound(time_ms(lambda: r.render_rows_device(p, d_out.data_ptr(), 4, 0, 1, stream, 0), warmup, launches),
                f"{form} NORMALS frame")
    if r.trace_path() != form:
        raise RuntimeError(f"asked for the {form} path kernel, ran {r.trace_path()}")
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.launches < 20:
        ap.error("--launches: at least 20")
    if not torch.cuda.is_available():
        sys.exit("ray_query_bench: no HIP device (this measurement has no CPU form)")
    torch.cuda.set_device(0)
    lines = [f"ray_query_bench: {args.width}x{args.height} = {args.width * args.height} rays, "
             f"{args.launches} launches after {args.warmup}, {torch.cuda.get_device_name(0)}"]
    bars = []
    for scene, forms in FORMS.items():
        r = wl.Renderer(scene, max_nodes=4096)
        scenes.build(scene, r)
        p = wl.render_params(args.width, args.height, spp=1, max_depth=1, mode=wl.MODE_NORMALS)
        rays = pixel_rays(r, p)
        ref = None
        for form in forms:
            q_ms, hit, hits = time_query(r, rays, form, args.warmup, args.launches)
            if ref is None:
                ref = hits
            elif hits.tobytes() != ref.tobytes():
                raise RuntimeError(f"{scene}: the {form} kernel's hits differ from the {forms[0]} kernel's")
            n_ms = time_normals(r, p, form, args.warmup, args.launches)
            ratio = q_ms / n_ms
            bars.append(ratio)
            lines.append(f"{scene:12s} pixel rays  {form:11s} query {q_ms:8.3f} ms  ({len(rays) / q_ms / 1e3:8.1f} "
                         f"Mrays/s, {hit:.3f} hit)   NORMALS frame {n_ms:8.3f} ms   query / frame {ratio:5.2f}")
        if scene == "rtiow_cover":
            inc = incoherent_rays(len(rays), INCOHERENT_BOX)
            ref = None
            for form in forms:
                q_ms, hit, hits = time_query(r, inc, form, args.warmup, args.launches)
                if ref is None:
                    ref = hits
                elif hits.tobytes() != ref.tobytes():
                    raise RuntimeError(f"{scene} incoherent: the {form} kernel's hits differ")
                lines.append(f"{scene:12s} incoherent  {form:11s} query {q_ms:8.3f} ms  ({len(inc) / q_ms / 1e3:8.1f} "
                             f"Mrays/s, {hit:.3f} hit)")
        r.close()
    lines.append(f"bar: query <= 1.25 x NORMALS frame of the same tracer: worst {max(bars):.2f} -> "
                 f"{'met' if max(bars) <= 1.25 else 'NOT met'}")
    text = "\n".join(lines + NOTES) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
