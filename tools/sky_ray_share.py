#!/usr/bin/env python3
"""The share of csg32's scattered rays that the sky-ray predicate (WO_SKY_RAYS, scene_jit.c
gen_sky_rays) accepts, by level, and what ending them at the scatter does to the frame time.

Share, on the GPU: the probe build (-DWO_SKY_RAYS_PROBE=1) runs the predicate where the
default build does but ends no path; it adds one to the segment counter per accepted ray.
With S the plain frame's segments and P its primary segments (pixels x spp), S - P rays
were scattered and went on, and

    p(level) = (segments of the level's probe build - S) / (S - P).

--cpu gives the same share from the CPU oracle over Lambertian scatters of the scene's
camera rays (the predicate compiled on the host, tests/test_sky_rays.py), with the share of
those rays that hit nothing.

--ab N times wo_renderer_render_rows_device (HIP events, prewarm, --frames frames a run) of
the listed levels in N alternating rounds.  Needs a GPU except with --cpu alone; not a
test, not bench.py.

    python tools/sky_ray_share.py --out profiles/sky_rays_before.txt
    python tools/sky_ray_share.py --ab 4 --levels 0,1,2

--take-probe counts, for the build --flags names, where the predicate's block runs and how full
the wave is there (probe builds WO_SKY_RAYS_PROBE 2..9, one count each); --variants times named
flag sets against each other, e.g. the thresholds of WO_SKY_RAYS_BOUNCE_MIN.

    python tools/sky_ray_share.py --take-probe --flags=-DWO_SKY_RAYS_BOUNCE_MIN=1 --out profiles/sky_rays_take_before.txt
    python tools/sky_ray_share.py --ab 4 --variants "all=-DWO_SKY_RAYS_BOUNCE_MIN=1;cam=-DWO_SKY_RAYS_BOUNCE_MIN=65"

--terms-probe compares levels on the same rays: each level's predicate runs in every iteration
with a lane that goes on and ends no path (probes 10..13), counted apart for camera and bounce
iterations; and it counts the bounce iterations that run once the tile's jobs are drained.

    python tools/sky_ray_share.py --terms-probe --levels 2,3 --out profiles/sky_rays_terms_before.txt
    python tools/sky_ray_share.py --terms-probe --levels 3,4 --out profiles/sky_rays_reach_before.txt

--levels takes every level the scene has (csg32: 1 to 4), in --terms-probe, --ab and --cpu.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cpu_share(say, n_cam, levels):
    """The predicate on the host against the oracle (the test's harness; a level it does not
    build itself, 3 or 4, from the same translation unit)."""
    import ctypes
    import pathlib
    import subprocess
    import tempfile

    import numpy as np
    import test_sky_rays as t

    tmp = pathlib.Path(tempfile.mkdtemp(prefix="sky_rays"))
    built = t.build_harness(tmp)
    levels = [L for L in levels if L > 0]
    for scene in t.SCENES:
        s = built[scene]
        for level in levels:
            if level not in s["libs"]:
                so = tmp / f"{scene}_{level}.so"
                subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC",
                                f"-DWO_SKY_RAYS={level}", "-I", os.path.join(ROOT, "include"), "-o", str(so),
                                str(tmp / f"{scene}.cpp")], check=True)
                s["libs"][level] = ctypes.CDLL(str(so))
        o, d = t._scattered(s, np.random.default_rng(1), n_cam)
        for level in levels:
            pred, hit, _ = t._check(s, level, o, d)
            say(f"cpu {scene} level {level}: {len(o)} scattered rays, {100.0 * (~hit).mean():.1f} % hit nothing, "
                f"predicate accepts {100.0 * pred.mean():.1f} %, accepted rays with a hit: {int((pred & hit).sum())}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="csg32")
    ap.add_argument("--levels", default="1,2")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--prewarm-s", type=float, default=0.3)
    ap.add_argument("--ab", type=int, default=0, help="alternating rounds timing the levels (0 included as listed)")
    ap.add_argument("--take-probe", action="store_true",
                    help="the predicate block's executions and lanes, the bounce and camera iterations (with --flags)")
    ap.add_argument("--terms-probe", action="store_true",
                    help="per level, the rays tested and accepted in camera and in bounce iterations with no path "
                         "ended, and the drained bounce iterations (with --flags)")
    ap.add_argument("--flags", default="", help="--take-probe, --terms-probe: the build's WOLOLO_JIT_FLAGS")
    ap.add_argument("--variants", default=None, help="time named flag sets: 'name=flags;name=flags' (rounds: --ab)")
    ap.add_argument("--cpu", action="store_true", help="the oracle's share too")
    ap.add_argument("--cpu-rays", type=int, default=20000, help="--cpu: camera rays")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    levels = [int(x) for x in a.levels.split(",")]
    if not a.no_gpu:
        import torch  # (before libwololo.so: one HIP runtime in the process)
        from csgrenderer_amd import scenes
        from csgrenderer_amd import wololo as wl

        def renderer(flags):
            os.environ["WOLOLO_JIT_FLAGS"] = flags
            r = wl.Renderer(a.scene, max_nodes=4096)
            info = scenes.build(a.scene, r)
            r.set_tracer("jit")
            r.prepare()
            return r, info.params()

        out = torch.zeros((1080, 1920, 4), dtype=torch.float32, device="cuda")
        seg = torch.zeros(1, dtype=torch.int64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def segments(r, p):
            seg.zero_()
            r.render_rows_device(p, out.data_ptr(), 4, 0, 1, stream, seg.data_ptr())
            torch.cuda.synchronize()
            return int(seg.item())

        def frame_ms(r, p):
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < a.prewarm_s:
                r.render_rows_device(p, out.data_ptr(), 4, 0, 1, stream, 0)
                torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.frames)]
            for x, y in ev:
                x.record()
                r.render_rows_device(p, out.data_ptr(), 4, 0, 1, stream, 0)
                y.record()
            torch.cuda.synchronize()
            return statistics.median(x.elapsed_time(y) for x, y in ev)

        if a.take_probe:
            # the loop's structure around the predicate's block, one probe build per count
            # (wo_device_common.h WO_SKY_RAYS_PROBE 2..9: each adds its count to the segments)
            r, p = renderer(a.flags)
            S, k = segments(r, p), r.kernel_info()
            r.close()
            say(f"{a.scene} {p.width}x{p.height} {p.spp} spp depth {p.max_depth}, flags '{a.flags}': {S} segments; kernel "
                f"{k['key'][:16]}, {k['vgprs']} VGPRs, {k['scratch_bytes']} B scratch, {k['lds_bytes']} B LDS")
            n = {}
            for kind in range(1, 10):
                r, p = renderer(f"{a.flags} -DWO_SKY_RAYS_PROBE={kind}")
                n[kind] = segments(r, p) - S
                r.close()

            def per(x, y):
                return f"{x / y:.2f}" if y else "-"

            say(f"predicate: {n[5] + n[4]} rays tested, {n[1]} accepted")
            say(f"(a) executions of the predicate's block: {n[2]} in camera iterations, {n[3]} in bounce iterations")
            say(f"(b) lanes under its mask: {n[4]} in camera iterations ({per(n[4], n[2])} a block), {n[5]} in bounce "
                f"iterations ({per(n[5], n[3])} a block); {per(n[4] + n[5], n[2] + n[3])} a block overall")
            say(f"(c) bounce iterations that trace: {n[6]}, busy lanes {n[7]} ({per(n[7], n[6])} a trace)")
            say(f"(d) camera iterations: {n[8]}, jobs {n[9]} ({per(n[9], n[8])} an iteration)")
        elif a.terms_probe:
            # per level: the predicate emitted in every iteration with a lane that goes on
            # (WO_SKY_RAYS_BOUNCE_MIN=1) and ending no path (probes 10..13), so every level
            # sees the same rays; then the drain's part of the bounce iterations (6, 7, 14, 15)
            r, p = renderer("-DWO_SKY_RAYS=0")
            S, P = segments(r, p), p.width * p.height * p.spp
            r.close()
            say(f"{a.scene} {p.width}x{p.height} {p.spp} spp depth {p.max_depth}: {S} segments, {P} primary")

            def count(flags, kind):
                r, p = renderer(f"{flags} -DWO_SKY_RAYS_PROBE={kind}")
                n = segments(r, p) - S
                r.close()
                return n

            share = {}
            for L in levels:
                f = f"-DWO_SKY_RAYS={L} -DWO_SKY_RAYS_BOUNCE_MIN=1"
                ca, ba, ct, bt = (count(f, k) for k in (10, 11, 12, 13))
                share[L] = ca / ct
                say(f"level {L}, ending none: camera iterations {ct} rays tested, {ca} accepted ({100.0 * ca / ct:.2f} %); "
                    f"bounce iterations {bt} continuing rays tested, {ba} accepted ({100.0 * ba / bt:.2f} %)")
            if len(levels) > 1:
                say(f"camera share, level {levels[-1]} / level {levels[0]}: {share[levels[-1]] / share[levels[0]]:.3f}")
            n = {k: count(a.flags, k) for k in (6, 7, 14, 15)}
            say(f"flags '{a.flags}': bounce iterations that trace {n[6]}, busy lanes {n[7]} ({n[7] / n[6]:.2f} a trace); of them "
                f"with the tile's jobs drained {n[14]}, busy lanes {n[15]} ({n[15] / max(n[14], 1):.2f} a trace); before the "
                f"drain {n[6] - n[14]}, busy lanes {n[7] - n[15]} ({(n[7] - n[15]) / max(n[6] - n[14], 1):.2f} a trace)")
        elif a.variants:
            # named flag sets against each other, as --ab does for the levels
            vs = [v.split("=", 1) for v in a.variants.split(";") if v]
            rs = [(name,) + renderer(flags) for name, flags in vs]
            say(f"{a.scene} {rs[0][2].width}x{rs[0][2].height} {rs[0][2].spp} spp depth {rs[0][2].max_depth}: median of "
                f"{a.frames} frames a run, {max(a.ab, 1)} alternating rounds")
            ms = {name: [] for name, _ in vs}
            for i in range(max(a.ab, 1)):
                for name, r, p in rs:
                    ms[name].append(frame_ms(r, p))
                say(f"round {i + 1}: " + ", ".join(f"{name} {ms[name][-1]:.4f} ms" for name, _ in vs))
            for (name, flags), (_, r, p) in zip(vs, rs):
                k = r.kernel_info()
                say(f"{name} ('{flags}'): median {statistics.median(ms[name]):.4f} ms, spread "
                    f"{max(ms[name]) - min(ms[name]):.4f}; kernel {k['key'][:16]}, {k['vgprs']} VGPRs, "
                    f"{k['scratch_bytes']} B scratch, {k['lds_bytes']} B LDS, {segments(r, p)} segments")
                r.close()
        elif a.ab:
            rs = [(L,) + renderer(f"-DWO_SKY_RAYS={L}") for L in levels]
            say(f"{a.scene} {rs[0][2].width}x{rs[0][2].height} {rs[0][2].spp} spp depth {rs[0][2].max_depth}: median of "
                f"{a.frames} frames a run, {a.ab} alternating rounds")
            ms = {L: [] for L in levels}
            for i in range(a.ab):
                for L, r, p in rs:
                    ms[L].append(frame_ms(r, p))
                say(f"round {i + 1}: " + ", ".join(f"level {L} {ms[L][-1]:.4f} ms" for L in levels))
            for L, r, p in rs:
                k = r.kernel_info()
                say(f"level {L}: median {statistics.median(ms[L]):.4f} ms, spread {max(ms[L]) - min(ms[L]):.4f}; kernel "
                    f"{k['key'][:16]}, {k['vgprs']} VGPRs, {k['scratch_bytes']} B scratch, {k['lds_bytes']} B LDS, "
                    f"{segments(r, p)} segments")
                r.close()
        else:
            r, p = renderer("-DWO_SKY_RAYS=0")
            S, P = segments(r, p), p.width * p.height * p.spp
            r.close()
            say(f"{a.scene} {p.width}x{p.height} {p.spp} spp depth {p.max_depth}: {S} segments, {P} primary, "
                f"{S - P} scattered rays that go on ({S / P:.4f} segments per path)")
            for L in levels:
                if L == 0:
                    continue
                r, p = renderer(f"-DWO_SKY_RAYS={L} -DWO_SKY_RAYS_PROBE=1")
                n = segments(r, p) - S
                say(f"gpu level {L}: the predicate accepts {n} of them, p = {100.0 * n / (S - P):.2f} %")
                r.close()
                r, p = renderer(f"-DWO_SKY_RAYS={L}")
                s2 = segments(r, p)
                say(f"gpu level {L}: the build that ends them counts {s2} segments ({'the same' if s2 == S else 'DIFFERENT'})")
                r.close()
    if a.cpu:
        os.environ.setdefault("WOLOLO_ALLOW_NO_DEVICE", "1")
        cpu_share(say, a.cpu_rays, levels)
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
