"""GPU: the tile pre-cull of the camera-ray waves (WO_CAM_TILE_CULL) never changes the
image.  Every frame below is bit-exact against the CPU oracle with the default build and
with -DWO_CAM_TILE_CULL=0, and the work counters show that the pre-cull acts."""
import numpy as np
import pytest

import pyoracle
from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl

pytestmark = pytest.mark.gpu

BUILDS = ["", "-DWO_CAM_TILE_CULL=0"]


def _same(gpu, ref, what):
    gpu, ref = np.asarray(gpu, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert gpu.shape == ref.shape, what
    d = np.where(np.isnan(gpu) & np.isnan(ref), 0.0, np.abs(gpu.astype(np.float64) - ref.astype(np.float64)))
    nbad = int((d > 0).sum())
    assert nbad == 0, f"{what}: not bit-exact ({nbad} values differ, max {float(d.max())})"


def _oracle(r, p):
    prog, nrec, _ = r.program()
    mats, nm = r.materials()
    return pyoracle.pathtrace_rows(prog, nrec, mats, nm, r.frame_desc(p), 0, p.height)[0]


def _both_builds(monkeypatch, scene, camera, check, **over):
    """`check(r, p, ref, what)` on a renderer of each build; the oracle's frame is made once."""
    ref = None
    for flags in BUILDS:
        monkeypatch.setenv("WOLOLO_JIT_FLAGS", flags)
        r = wl.Renderer(scene, max_nodes=4096)
        info = scenes.build(scene, r)
        if camera:
            r.set_camera(*camera)
        r.set_tracer("jit")
        p = info.params(**over)
        if ref is None:
            ref = _oracle(r, p)
        check(r, p, ref, f"{scene} {over} camera={camera} flags='{flags}'")
        assert r.trace_path() == "jit"
        has_table = "kTileBound" in r.jit_source()
        assert has_table == (scene == "csg32")  # term mode with the spatial hierarchy
        r.close()


def _render_equals(r, p, ref, what):
    _same(r.render(p), ref, what)


@pytest.mark.parametrize("mode", [wl.MODE_PATHTRACE, wl.MODE_NORMALS])
@pytest.mark.parametrize("scene", ["csg32", "csg256_balanced"])
def test_small_frame_bitexact_both_builds(scene, mode, monkeypatch):
    """csg32 (the pre-cull's kernel) and csg256_balanced (the union count: no table, the
    switch changes nothing) at 96x54, 4 spp, depth 8."""
    _both_builds(monkeypatch, scene, None, _render_equals, width=96, height=54,
                 spp=4 if mode == wl.MODE_PATHTRACE else 1, max_depth=8, mode=mode, seed=7)


@pytest.mark.parametrize("w,h", [(61, 35), (13, 7)])
def test_partial_tiles_bitexact_both_builds(w, h, monkeypatch):
    """61x35: partial tiles in both directions; 13x7: the small tail tiles only."""
    _both_builds(monkeypatch, "csg32", None, _render_equals, width=w, height=h, spp=4, max_depth=8, seed=3)


def test_three_ranks_four_row_tiles_both_builds(monkeypatch):
    """csg32 in 3 ranks' 4-row tiles (a tile's frame rows come through the band mapping),
    assembled: equal to the one-rank frame, which equals the oracle's."""
    import torch

    def check(r, p, ref, what):
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

    _both_builds(monkeypatch, "csg32", None, check, width=61, height=35, spp=2, max_depth=8, seed=5)


CAMERAS = {
    # (look_from, look_at, vup, vfov, aperture, focus_dist)
    "inside the crater sphere, above the slab": ((2.5, 0.5, 1.5), (0.0, 0.6, 0.0), (0, 1, 0), 60.0, 0.0, 1.0),
    "inside the crater sphere and the slab's box": ((2.3, -0.1, 1.4), (0.0, 1.5, -1.0), (0, 1, 0), 70.0, 0.0, 1.0),
    "inside a group sphere": ((-1.9, 1.3, 2.7), (0.0, 0.6, 0.0), (0, 1, 0), 55.0, 0.0, 1.0),
    "all geometry behind the camera": ((0.0, 4.5, 10.0), (0.0, 9.0, 20.0), (0, 1, 0), 45.0, 0.0, 10.0),
    "aperture 0.1 (pre-cull disabled)": ((0.0, 4.5, 10.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0, 0.1, 10.0),
}


@pytest.mark.parametrize("name", list(CAMERAS))
def test_cameras_bitexact_both_builds(name, monkeypatch):
    def check(r, p, ref, what):
        img = r.render(p)
        _same(img, ref, what)
        if name.startswith("all geometry behind"):
            sky = np.asarray(ref)[..., :3]
            assert (sky[..., 2] >= sky[..., 0]).all() and np.isfinite(sky).all()  # the sky gradient alone

    _both_builds(monkeypatch, "csg32", CAMERAS[name], check, width=96, height=54, spp=4, max_depth=8, seed=11)


def test_work_counters_show_the_pre_cull(monkeypatch):
    """csg32 at 96x54: the same segments with the switch on and off (no path changes), and
    fewer wave-level bound tests and sphere tests per segment with it on."""
    work = {}
    for flags in BUILDS:
        monkeypatch.setenv("WOLOLO_JIT_FLAGS", flags)
        r = wl.Renderer("csg32", max_nodes=4096)
        info = scenes.build("csg32", r)
        r.set_tracer("jit")
        work[flags] = r.count_work(info.params(width=96, height=54, spp=4, max_depth=8, seed=7))
        r.close()
    on, off = work[BUILDS[0]], work[BUILDS[1]]
    print({k: (on[k], off[k]) for k in ("segments", "bound_tests", "sphere_tests", "halfspace_tests")})
    assert on["segments"] == off["segments"] > 0
    assert on["bound_tests"] / on["segments"] < off["bound_tests"] / off["segments"]
    assert on["sphere_tests"] <= off["sphere_tests"] and on["halfspace_tests"] <= off["halfspace_tests"]
    assert on["sweep_steps"] == off["sweep_steps"] and on["primary_segments"] == off["primary_segments"]
