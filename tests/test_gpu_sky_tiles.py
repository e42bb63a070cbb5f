"""GPU: tiles whose pre-cull leaves nothing to trace are rendered by a direct sky loop
(WO_CAM_SKY_TILES) instead of the path loop, and the image never changes.  Every frame
below is bit-exact against the CPU oracle with the default build and with
-DWO_CAM_SKY_TILES=0, the two builds load different kernels, and their work counters are
the same."""
import ctypes

import numpy as np
import pytest

import pyoracle
import test_tile_cull as tc
from test_tile_cull import harness  # noqa: F401  (the host build of tile_frustum / tile_culls)
from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl

pytestmark = pytest.mark.gpu

BUILDS = ["", "-DWO_CAM_SKY_TILES=0"]
# tests/test_gpu_tile_cull.py's cameras: (look_from, look_at, vup, vfov, aperture, focus_dist)
BEHIND = ((0.0, 4.5, 10.0), (0.0, 9.0, 20.0), (0, 1, 0), 45.0, 0.0, 10.0)  # all geometry behind the camera
LENS = ((0.0, 4.5, 10.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0, 0.1, 10.0)     # aperture 0.1: the pre-cull is off


def _same(gpu, ref, what):
    gpu, ref = np.asarray(gpu, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert gpu.shape == ref.shape, what
    d = np.where(np.isnan(gpu) & np.isnan(ref), 0.0, np.abs(gpu.astype(np.float64) - ref.astype(np.float64)))
    nbad = int((d > 0).sum())
    assert nbad == 0, f"{what}: not bit-exact ({nbad} values differ, max {float(d.max())})"


def _oracle(r, p):
    prog, nrec, _ = r.program()
    mats, nm = r.materials()
    return pyoracle.pathtrace_rows(prog, nrec, mats, nm, r.frame_desc(p), 0, p.height)


def _both_builds(monkeypatch, camera, check, **over):
    """`check(r, p, ref, segs, what)` on a csg32 renderer of each build; the oracle's frame
    is made once, and the two builds' loaded kernels differ (the flag took effect)."""
    ref, keys = None, []
    for flags in BUILDS:
        monkeypatch.setenv("WOLOLO_JIT_FLAGS", flags)
        r = wl.Renderer("csg32", max_nodes=4096)
        info = scenes.build("csg32", r)
        if camera:
            r.set_camera(*camera)
        r.set_tracer("jit")
        p = info.params(**over)
        if ref is None:
            ref = _oracle(r, p)
        check(r, p, ref[0], ref[1], f"csg32 {over} camera={camera} flags='{flags}'")
        assert r.trace_path() == "jit"
        assert "tile_all_culled" in r.jit_source()
        keys.append(r.kernel_info()["key"])
        r.close()
    assert keys[0] != keys[1], keys


def _render_equals(r, p, ref, segs, what):
    _same(r.render(p), ref, what)


def _rows_and_segments(r, p, ref, segs, what):
    """The frame through render_rows_device with its segment counter: one per sample."""
    import torch
    out = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device="cuda")
    seg = torch.zeros(1, dtype=torch.int64, device="cuda")
    r.render_rows_device(p, out.data_ptr(), 16, 0, 1, torch.cuda.current_stream().cuda_stream, seg.data_ptr())
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), ref, what)
    spp = p.spp if p.mode == wl.MODE_PATHTRACE else 1
    assert int(seg.item()) == p.width * p.height * spp == segs, what


@pytest.mark.parametrize("spp", [1, 3, 5, 8])
def test_all_sky_frame_pathtrace(spp, monkeypatch):
    """Every tile is a sky tile; spp 1, 3, 5, 8: job counts that do not divide over the
    4 waves or the 256 threads (a 64-pixel tile has 64, 192, 320 and 512 jobs)."""
    _both_builds(monkeypatch, BEHIND, _rows_and_segments, width=96, height=54, spp=spp, max_depth=8, seed=11)


def test_all_sky_frame_normals(monkeypatch):
    _both_builds(monkeypatch, BEHIND, _rows_and_segments, width=96, height=54, spp=1, max_depth=8,
                 mode=wl.MODE_NORMALS, seed=11)


@pytest.mark.parametrize("w,h", [(61, 35), (13, 7), (1, 1)])
def test_all_sky_partial_tiles(w, h, monkeypatch):
    """61x35: partial tiles in both directions; 13x7: 4x4 tail tiles only; 1x1: one pixel."""
    _both_builds(monkeypatch, BEHIND, _rows_and_segments, width=w, height=h, spp=5, max_depth=8, seed=3)


MIXED = (96, 54)


def test_mixed_frame_has_sky_tiles_and_traced_tiles(harness, monkeypatch):  # noqa: F811
    """csg32's own camera at 96x54, 4 spp: by the prologue's test compiled on the host, tiles
    of every shape a launch forms cull every entry and others do not; the frame is bit-exact."""
    def check(r, p, ref, segs, what):
        entries = tc._table(r.jit_source())
        tab, n = tc._ctable(entries), len(entries)
        fr = r.frame_desc(p)
        tiles = tc._tiles(p.width, p.height)
        masks = np.zeros(len(tiles), dtype=np.uint64)
        harness.tile_masks(ctypes.byref(fr.cam), ctypes.c_float(fr.inv_width), ctypes.c_float(fr.inv_height),
                           ctypes.c_uint32(p.height), tc._ptr(tiles), ctypes.c_uint32(len(tiles)), tab,
                           ctypes.c_uint32(n), tc._ptr(masks))
        allc = masks == np.uint64((1 << n) - 1)
        tw, th = tiles[:, 1] - tiles[:, 0], tiles[:, 3] - tiles[:, 2] + 1
        for sw, sh in ((8, 8), (8, 4), (4, 4)):
            shape = (tw == sw) & (th == sh)
            assert (allc & shape).any() and (~allc & shape).any(), (what, sw, sh)
        _same(r.render(p), ref, what)
        assert segs > p.width * p.height * p.spp  # some paths bounce

    _both_builds(monkeypatch, None, check, width=MIXED[0], height=MIXED[1], spp=4, max_depth=8, seed=7)


def test_three_ranks_four_row_tiles(monkeypatch):
    """3 ranks' 4-row tiles at 61x35 (a tile's frame rows come through the band mapping),
    assembled: equal to the one-rank frame, which equals the oracle's."""
    import torch

    def check(r, p, ref, segs, what):
        full = r.render(p)
        _same(full, ref, what)
        nranks, tile = 3, 4
        lr = wl.local_rows(p.height, tile, nranks)
        gathered = torch.zeros((nranks, lr, p.width, 4), dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for rank in range(nranks):
            r.render_rows_device(p, gathered[rank].data_ptr(), tile, rank, nranks, stream, 0)
        frame = torch.empty((p.height, p.width, 4), dtype=torch.float32, device="cuda")
        wl.assemble_rows_device(gathered.data_ptr(), frame.data_ptr(), p.width, p.height, tile, nranks, stream)
        torch.cuda.synchronize()
        assert np.array_equal(frame.cpu().numpy(), full), what

    _both_builds(monkeypatch, BEHIND, check, width=61, height=35, spp=3, max_depth=8, seed=5)


def test_progressive_accumulation_over_sky_tiles(monkeypatch):
    """Two accumulated launches of 2 spp == one render of 4 spp, from a non-zero sample
    offset (the second launch's samples follow the first's)."""
    def check(r, p, ref, segs, what):
        half = wl.render_params(p.width, p.height, spp=2, max_depth=p.max_depth, seed=p.seed, mode=p.mode,
                                sample_offset=p.sample_offset)
        img, n = r.render_accumulate(half, reset=True)
        assert n == 2
        img, n = r.render_accumulate(half)
        assert n == 4
        _same(img, ref, what + " 2 x 2 spp")
        _same(r.render(p), ref, what)

    _both_builds(monkeypatch, BEHIND, check, width=61, height=35, spp=4, max_depth=8, seed=9, sample_offset=5)


@pytest.mark.parametrize("camera", [BEHIND, None], ids=["all sky", "own camera"])
def test_work_counters_equal_with_the_flag_on_and_off(camera, monkeypatch):
    work = {}
    for flags in BUILDS:
        monkeypatch.setenv("WOLOLO_JIT_FLAGS", flags)
        r = wl.Renderer("csg32", max_nodes=4096)
        info = scenes.build("csg32", r)
        if camera:
            r.set_camera(*camera)
        r.set_tracer("jit")
        work[flags] = r.count_work(info.params(width=96, height=54, spp=5, max_depth=8, seed=7))
        r.close()
    on, off = work[BUILDS[0]], work[BUILDS[1]]
    kinds = ("segments", "primary_segments", "sphere_tests", "halfspace_tests", "bound_tests", "idle_lanes")
    print({k: (on[k], off[k]) for k in kinds})
    # With the scene's own camera the traced tiles' waves share their tile's job queue in
    # the order their atomics arrive, so which jobs meet in a wave -- its wave-level tests
    # and idle lanes -- is not determined even between two runs of ONE build; the segments
    # are.  The all-sky frame traces nothing and every count is determined.
    for k in (kinds if camera else kinds[:2]):
        assert on[k] == off[k], k
    assert on["primary_segments"] == 96 * 54 * 5
    if camera:
        assert on["segments"] == 96 * 54 * 5
        assert on["sphere_tests"] == on["halfspace_tests"] == on["bound_tests"] == on["idle_lanes"] == 0


def test_aperture_never_takes_the_sky_loop(monkeypatch):
    """With a lens the pre-cull words are all 0 and the loop is never taken: bit-exact."""
    _both_builds(monkeypatch, LENS, _render_equals, width=96, height=54, spp=4, max_depth=8, seed=11)
