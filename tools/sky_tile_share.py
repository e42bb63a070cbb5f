#!/usr/bin/env python3
"""What the tiles whose pre-cull leaves nothing to trace (sky tiles) cost csg32's 1080p64
frame, and what the direct sky loop (WO_CAM_SKY_TILES) makes of them.

Times wo_renderer_render_rows_device of csg32 at 1920x1080, 64 spp, depth 8 with HIP events
(prewarm, then --frames frames) for two cameras: the scene's own, and the "all geometry
behind the camera" camera of tests/test_gpu_tile_cull.py, in which every tile is a sky tile.

    share = (all-sky frame time) x (sky tiles / tiles of the scene's frame) / (scene's frame time)

is the share of the scene's frame its sky tiles take (6 053 of 32 400 8x8 tiles with the
scene's camera).  --flags sets the kernel's build (WOLOLO_JIT_FLAGS), e.g.
"-DWO_CAM_SKY_TILES=0" for the path loop in every tile.  --ab N instead times the all-sky
frame with the default build and with -DWO_CAM_SKY_TILES=0 in N alternating pairs.
Needs a GPU; not a test, not bench.py.

    python tools/sky_tile_share.py --flags=-DWO_CAM_SKY_TILES=0 --out profiles/sky_tiles_before.txt
    python tools/sky_tile_share.py --ab 4
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before libwololo.so: one HIP runtime in the process)

from csgrenderer_amd import scenes  # noqa: E402
from csgrenderer_amd import wololo as wl  # noqa: E402

BEHIND = ((0.0, 4.5, 10.0), (0.0, 9.0, 20.0), (0, 1, 0), 45.0, 0.0, 10.0)  # tests/test_gpu_tile_cull.py CAMERAS
SKY_TILES, TILES = 6053, 32400  # csg32's camera at 1920x1080, 8x8 tiles (tests/test_tile_cull.py prints them)


def renderer(flags, camera, spp=64):
    os.environ["WOLOLO_JIT_FLAGS"] = flags
    r = wl.Renderer("csg32", max_nodes=4096)
    info = scenes.build("csg32", r)
    if camera:
        r.set_camera(*camera)
    r.set_tracer("jit")
    r.prepare()
    return r, info.params(spp=spp)


def frame_ms(r, p, out, seg, frames, prewarm_s):
    """Mean HIP-event time of `frames` launches after `prewarm_s` of untimed ones; also the
    segments of one launch."""
    stream = torch.cuda.current_stream().cuda_stream
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < prewarm_s:
        r.render_rows_device(p, out.data_ptr(), 4, 0, 1, stream, 0)
        torch.cuda.synchronize()
    seg.zero_()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(frames)]
    for a, b in ev:
        a.record()
        r.render_rows_device(p, out.data_ptr(), 4, 0, 1, stream, seg.data_ptr())
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return sum(ms) / frames, min(ms), max(ms), int(seg.item()) // frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flags", default="", help="WOLOLO_JIT_FLAGS of the kernel")
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--prewarm-s", type=float, default=0.3)
    ap.add_argument("--spp", type=int, default=64, help="--ab: samples per pixel (a small count shows the workgroup's "
                                                        "set-up and write-out, which the loop does not change)")
    ap.add_argument("--ab", type=int, default=0, help="alternating pairs of the all-sky frame, default build against "
                                                      "-DWO_CAM_SKY_TILES=0")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    out = torch.zeros((1080, 1920, 4), dtype=torch.float32, device="cuda")
    seg = torch.zeros(1, dtype=torch.int64, device="cuda")
    if a.ab:
        builds = [("WO_CAM_SKY_TILES=1", ""), ("WO_CAM_SKY_TILES=0", "-DWO_CAM_SKY_TILES=0")]
        rs = [(name,) + renderer(flags, BEHIND, a.spp) for name, flags in builds]
        say(f"csg32 1920x1080 {a.spp} spp, all geometry behind the camera (every tile a sky tile), {a.frames} frames a run")
        wins = 0
        for i in range(a.ab):
            t = {}
            for name, r, p in rs:
                t[name] = frame_ms(r, p, out, seg, a.frames, a.prewarm_s)
                say(f"pair {i + 1} {name}: {t[name][0]:.4f} ms (min {t[name][1]:.4f}, max {t[name][2]:.4f}), "
                    f"{t[name][3]} segments")
            on, off = t[builds[0][0]][0], t[builds[1][0]][0]
            wins += on < off
            say(f"pair {i + 1} ratio off / on: {off / on:.3f}")
        for name, r, _ in rs:
            say(f"{name}: kernel {r.kernel_info()['key'][:16]}, {r.kernel_info()['vgprs']} VGPRs")
        say(f"the sky loop is faster in {wins} of {a.ab} pairs")
    else:
        say(f"csg32 1920x1080 64 spp depth 8, WOLOLO_JIT_FLAGS='{a.flags}', {a.frames} frames a run")
        t = {}
        for name, cam in (("scene camera", None), ("all-sky camera", BEHIND)):
            r, p = renderer(a.flags, cam)
            t[name] = frame_ms(r, p, out, seg, a.frames, a.prewarm_s)
            say(f"{name}: {t[name][0]:.4f} ms (min {t[name][1]:.4f}, max {t[name][2]:.4f}), {t[name][3]} segments, "
                f"kernel {r.kernel_info()['key'][:16]}")
            r.close()
        share = t["all-sky camera"][0] * SKY_TILES / TILES / t["scene camera"][0]
        say(f"sky tiles' share of the scene's frame: {t['all-sky camera'][0]:.4f} x {SKY_TILES} / {TILES} / "
            f"{t['scene camera'][0]:.4f} = {100.0 * share:.2f} %")
    if a.out:
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
