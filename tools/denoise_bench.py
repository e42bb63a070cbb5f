#!/usr/bin/env python3
"""Time the a-trous denoiser (wo_denoise_device) at 1920x1080 on csg32 at 4 spp, the frame and its
feature planes rendered on the GPU, with the default parameters (5 levels):

  (a) the whole denoise (prologue + 5 levels), as `auto` dispatches it and with each form forced;
  (b) each level alone (WOLOLO_DENOISE_ONLY_LEVEL) in the direct form and, at the steps that have
      one, in the LDS form -- the per-level rule of `auto` keeps the faster;
  (c) as a floor, device-to-device copies in the same process: of 48 B per pixel (a level reads two
      16-byte rows per pixel and writes one) and of 24 B per pixel (a copy reads and writes, so this
      one moves the 48 B a level cannot avoid);
  (d) for context the 4-spp frame (wo_renderer_render_rows_device, the kernel AUTO picks) and the
      feature pass (wo_renderer_render_features_device).

HIP events, `--launches` launches per variant after `--warmup`, the variants alternating in
`--rounds` rounds inside one process; per variant the median round and the spread (min .. max).
Needs a GPU; not a test, not bench.py.

    python tools/denoise_bench.py --out profiles/denoise_bench.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (before libwololo.so: one HIP runtime in the process)

import feature_bench as fb  # noqa: E402
from csgrenderer_amd import scenes  # noqa: E402
from csgrenderer_amd import wololo as wl  # noqa: E402

LDS_MAX_STEP = 4  # denoise_kernels.hip kLdsMaxStep


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--scene", default="csg32")
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("denoise_bench: no HIP device (this measurement has no CPU form)")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    w, h = args.width, args.height
    n = w * h
    r = wl.Renderer(args.scene, max_nodes=4096)
    scenes.build(args.scene, r)
    r.prepare()
    p = wl.render_params(w, h, spp=args.spp, seed=1, mode=wl.MODE_PATHTRACE)
    rows = wl.local_rows(h, 16, 1)
    d_frame = torch.zeros((rows * w, 4), dtype=torch.float32, device="cuda")
    d_planes = torch.zeros((3 * n, 4), dtype=torch.int32, device="cuda")
    dp = wl.denoise_params()
    need = wl.denoise_scratch_bytes(w, h, dp)
    d_out = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    d_scratch = torch.zeros(need // 4, dtype=torch.int32, device="cuda")
    plane = lambda k: d_planes.data_ptr() + k * n * 16  # noqa: E731

    def frame():
        r.render_rows_device(p, d_frame.data_ptr(), 16, 0, 1, stream)

    def features():
        r.render_features_device(p, d_planes.data_ptr(), n, h, 0, 1, stream)

    def denoise(form, only=None):
        def fn():
            os.environ["WOLOLO_DENOISE_FORM"] = form
            if only is None:
                os.environ.pop("WOLOLO_DENOISE_ONLY_LEVEL", None)
            else:
                os.environ["WOLOLO_DENOISE_ONLY_LEVEL"] = str(only)
            wl.denoise_device(dp, w, h, d_frame.data_ptr(), plane(0), plane(1), plane(2), d_out.data_ptr(),
                              d_scratch.data_ptr(), need, stream)
        return fn

    def copy_of(bytes_per_pixel):
        src = torch.zeros(n * bytes_per_pixel // 4, dtype=torch.int32, device="cuda")
        dst = torch.zeros_like(src)
        return lambda: dst.copy_(src)

    frame()
    features()
    # every form gives the same frame
    ref = None
    for form in ("direct", "lds", "auto"):
        d_out.zero_()
        denoise(form)()
        torch.cuda.synchronize()
        got = d_out.cpu().numpy().tobytes()
        if ref is None:
            ref = got
        elif got != ref:
            raise RuntimeError(f"form {form} gives another frame than direct")
    variants = {("whole", f): denoise(f) for f in ("auto", "direct", "lds")}
    for level in range(dp.levels):
        variants[("level", level, "direct")] = denoise("direct", level)
        if (1 << level) <= LDS_MAX_STEP:
            variants[("level", level, "lds")] = denoise("lds", level)
    variants[("copy", 48)] = copy_of(48)
    variants[("copy", 24)] = copy_of(24)
    variants[("frame",)] = frame
    variants[("features",)] = features
    ms = fb.time_rounds(variants, args.warmup, args.launches, args.rounds, "denoise")
    os.environ.pop("WOLOLO_DENOISE_FORM", None)
    os.environ.pop("WOLOLO_DENOISE_ONLY_LEVEL", None)

    def fmt(key):
        m, lo, hi = ms[key]
        return f"{m:8.4f} ms ({lo:.4f} .. {hi:.4f})"

    c48, c24 = ms[("copy", 48)][0], ms[("copy", 24)][0]
    lines = [f"denoise_bench: {args.scene} {w}x{h} = {n} pixels at {args.spp} spp, defaults ({dp.levels} levels), "
             f"{args.launches} launches per variant after {args.warmup} in {args.rounds} alternating rounds, "
             f"{torch.cuda.get_device_name(0)}",
             "ms per launch: median round (min .. max over the rounds)",
             f"(c) floor: copy of 48 B per pixel {fmt(('copy', 48))}, {48 * n / c48 * 1e-9:6.2f} TB/s copied; "
             f"of 24 B per pixel {fmt(('copy', 24))}",
             f"(d) context: frame on \"{r.trace_path()}\" {fmt(('frame',))}; feature pass {fmt(('features',))}"]
    for f in ("auto", "direct", "lds"):
        a = ms[("whole", f)][0]
        lines.append(f"(a) whole denoise, {f:6s} {fmt(('whole', f))}; / ({dp.levels} x copy of 48 B) = {a / (dp.levels * c48):5.2f}, "
                     f"/ ({dp.levels} x copy of 24 B) = {a / (dp.levels * c24):5.2f}")
    switch = None
    for level in range(dp.levels):
        d = ms[("level", level, "direct")][0]
        line = f"(b) level {level} (step {1 << level:2d}) alone: direct {fmt(('level', level, 'direct'))}, {d / c48:5.2f} x copy48"
        if ("level", level, "lds") in ms:
            l = ms[("level", level, "lds")][0]
            line += f"; lds {fmt(('level', level, 'lds'))}, {l / c48:5.2f} x copy48; lds / direct = {l / d:5.2f}"
            if l < d:
                switch = 1 << level
        else:
            line += "; no lds form at this step"
        lines.append(line)
    lines.append("rule: the LDS form is faster at no step" if switch is None else
                 f"rule: the LDS form is faster up to step {switch}")
    text = "\n".join(lines + fb.NOTES) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    r.close()


if __name__ == "__main__":
    main()
