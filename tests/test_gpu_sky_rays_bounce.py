"""GPU: in which iterations the sky-ray predicate runs (WO_SKY_RAYS_BOUNCE_MIN: a bounce
iteration tests only from that many lanes that go on; 1 in every iteration, 65 in camera
iterations only, the default) changes neither the image nor the segment count: an untested
ray is simply traced.  Every frame below is bit-exact against the CPU oracle, with the
oracle's segment count, for thresholds 1 and 65 crossed with the predicate's levels 1 and 2,
and for a threshold in between; the builds load different kernels, none uses scratch, and
their LDS is the same.

The shapes are the smallest at which the loop's control flow can go wrong: a wave with a
single lane, more jobs than ring slots (the ring wraps), partial tiles, depths at which no
ray or only last segments go on, cameras for which the predicate ends nearly every
continuing ray (the ring stays nearly empty) or nearly none."""
import numpy as np
import pytest

import pyoracle
from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl

pytestmark = pytest.mark.gpu

BUILDS = [f"-DWO_SKY_RAYS_BOUNCE_MIN={k} -DWO_SKY_RAYS={level}" for k in (1, 65) for level in (1, 2)] + [
    "-DWO_SKY_RAYS_BOUNCE_MIN=24"]
# (look_from, look_at, vup, vfov, aperture, focus_dist)
FLOOR_UP = ((1.0, 0.0, 5.0), (0.0, 3.0, 0.0), (0, 1, 0), 60.0, 0.0, 10.0)      # on the slab's top face, looking up
IN_GROUP1 = ((0.3, 1.2, 2.4), (0.0, 0.8, -1.0), (0, 1, 0), 70.0, 0.0, 10.0)   # at group 1's centre (R = 3.1)
IN_SLAB = ((3.0, -0.25, -3.0), (0.0, 1.0, 0.0), (0, 1, 0), 60.0, 0.0, 10.0)    # inside the slab's box
BEHIND = ((0.0, 4.5, 10.0), (0.0, 9.0, 20.0), (0, 1, 0), 45.0, 0.0, 10.0)      # all geometry behind the camera
LENS = ((0.0, 4.5, 10.0), (0.0, 0.6, 0.0), (0, 1, 0), 45.0, 0.1, 10.0)         # aperture 0.1
CAMERAS = {"floor up": FLOOR_UP, "in group 1": IN_GROUP1, "in slab": IN_SLAB, "behind": BEHIND, "lens": LENS}


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


def _all_builds(monkeypatch, scene, camera, check, builds=BUILDS, **over):
    """`check(r, p, ref, segs, what)` on a renderer of each build; the oracle's frame and
    segment count are made once.  Returns the builds' kernel_info."""
    ref, infos = None, []
    for flags in builds:
        monkeypatch.setenv("WOLOLO_JIT_FLAGS", flags)
        r = wl.Renderer(scene, max_nodes=4096)
        info = scenes.build(scene, r)
        if camera:
            r.set_camera(*camera)
        r.set_tracer("jit")
        p = info.params(**over)
        if ref is None:
            ref = _oracle(r, p)
        check(r, p, ref[0], ref[1], f"{scene} {over} camera={camera} flags='{flags}'")
        assert r.trace_path() == "jit"
        infos.append(r.kernel_info())
        r.close()
    return infos


def _resources(infos):
    """Five builds: five kernels (so the thresholds differ at either level), none with
    scratch, one LDS size."""
    assert len({i["key"] for i in infos}) == len(infos) == len(BUILDS), infos
    assert [i["scratch_bytes"] for i in infos] == [0] * len(BUILDS), infos
    assert len({i["lds_bytes"] for i in infos}) == 1, infos


def _rows_and_segments(r, p, ref, segs, what):
    """The frame through render_rows_device with its segment counter."""
    import torch
    out = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device="cuda")
    seg = torch.zeros(1, dtype=torch.int64, device="cuda")
    r.render_rows_device(p, out.data_ptr(), 16, 0, 1, torch.cuda.current_stream().cuda_stream, seg.data_ptr())
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), ref, what)
    assert int(seg.item()) == segs, (what, int(seg.item()), segs)


@pytest.mark.parametrize("spp", [1, 3, 5, 8])
def test_csg32_own_camera_spp(spp, monkeypatch):
    infos = _all_builds(monkeypatch, "csg32", None, _rows_and_segments, width=96, height=54, spp=spp, max_depth=8,
                        seed=11)
    _resources(infos)
    assert infos[0]["lds_bytes"] == 17912, infos  # no LDS beside the block's ring, sums, frame copy and records


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_csg32_depths(depth, monkeypatch):
    """Depth 1: no ray goes on, the block never finds a lane; depth 2: every continuing ray is
    at its last segment; depth 3: the first with rays that leave a bounce iteration untested."""
    def check(r, p, ref, segs, what):
        _rows_and_segments(r, p, ref, segs, what)
        if depth == 1:
            assert segs == p.width * p.height * p.spp
        else:
            assert segs > p.width * p.height * p.spp
    _resources(_all_builds(monkeypatch, "csg32", None, check, width=96, height=54, spp=4, max_depth=depth, seed=7))


@pytest.mark.parametrize("spp", [1, 130, 400])
def test_csg32_single_pixel(spp, monkeypatch):
    """1 x 1.  1 spp: a single lane, whose only ray the test may end (nothing to push);
    130 spp: more jobs than the ring's 64 slots, and a camera iteration of 2 jobs; 400 spp:
    more jobs than the four waves' first camera iterations take, so a wave's second one
    pushes behind a moved head and the ring wraps."""
    _all_builds(monkeypatch, "csg32", None, _rows_and_segments, width=1, height=1, spp=spp, max_depth=8, seed=3)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_csg32_single_sample_seeds(seed, monkeypatch):
    """1 x 1, 1 spp over seeds: paths that miss at once, scatter into the sky, or go on."""
    _all_builds(monkeypatch, "csg32", None, _rows_and_segments, width=1, height=1, spp=1, max_depth=8, seed=seed)


@pytest.mark.parametrize("w,h", [(13, 7), (61, 35)])
def test_csg32_partial_tiles(w, h, monkeypatch):
    _all_builds(monkeypatch, "csg32", None, _rows_and_segments, width=w, height=h, spp=5, max_depth=8, seed=3)


@pytest.mark.parametrize("camera", list(CAMERAS), ids=[c.replace(" ", "_") for c in CAMERAS])
def test_csg32_cameras(camera, monkeypatch):
    """Floor up: nearly every continuing ray is ended by the test, so little reaches the
    ring; in group 1 and in the slab: almost none is; behind: nothing scatters; a lens."""
    def check(r, p, ref, segs, what):
        _rows_and_segments(r, p, ref, segs, what)
        if camera == "behind":
            assert segs == p.width * p.height * p.spp  # nothing is hit, nothing scatters
        else:
            assert segs > p.width * p.height * p.spp
    _all_builds(monkeypatch, "csg32", CAMERAS[camera], check, width=96, height=54, spp=4, max_depth=8, seed=11)


def test_csg32_union(monkeypatch):
    _resources(_all_builds(monkeypatch, "csg32_union", None, _rows_and_segments, width=96, height=54, spp=4,
                           max_depth=8, seed=7))


def test_three_ranks_four_row_tiles(monkeypatch):
    """3 ranks' 4-row tiles at 61x35, assembled: the one-rank frame, which is the oracle's."""
    import torch

    def check(r, p, ref, segs, what):
        full = r.render(p)
        _same(full, ref, what)
        nranks, tile = 3, 4
        lr = wl.local_rows(p.height, tile, nranks)
        gathered = torch.zeros((nranks, lr, p.width, 4), dtype=torch.float32, device="cuda")
        seg = torch.zeros(1, dtype=torch.int64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for rank in range(nranks):
            r.render_rows_device(p, gathered[rank].data_ptr(), tile, rank, nranks, stream, seg.data_ptr())
        frame = torch.empty((p.height, p.width, 4), dtype=torch.float32, device="cuda")
        wl.assemble_rows_device(gathered.data_ptr(), frame.data_ptr(), p.width, p.height, tile, nranks, stream)
        torch.cuda.synchronize()
        assert np.array_equal(frame.cpu().numpy(), full), what
        assert int(seg.item()) == segs, what  # the ranks' segments add up to the frame's

    _all_builds(monkeypatch, "csg32", None, check, width=61, height=35, spp=3, max_depth=8, seed=5)


def test_progressive_accumulation(monkeypatch):
    """Two accumulated launches of 4 spp == one render of 8 spp, from a non-zero sample offset."""
    def check(r, p, ref, segs, what):
        half = wl.render_params(p.width, p.height, spp=4, max_depth=p.max_depth, seed=p.seed, mode=p.mode,
                                sample_offset=p.sample_offset)
        img, n = r.render_accumulate(half, reset=True)
        assert n == 4
        img, n = r.render_accumulate(half)
        assert n == 8
        _same(img, ref, what + " 2 x 4 spp")
        _same(r.render(p), ref, what)

    _all_builds(monkeypatch, "csg32", None, check, width=61, height=35, spp=8, max_depth=8, seed=9, sample_offset=5)


def test_csg32_nested_is_untouched(monkeypatch):
    """A form without the predicate.  The code-object key hashes the compile options, so it
    differs with the flags even where they change nothing; that the kernel is the same shows
    in its source, which names no such switch, and in a code object of the same size and
    resources under each flag as without them, with the frame bit-exact as before."""
    sizes = []

    def check(r, p, ref, segs, what):
        src = r.jit_source()
        assert "ray_misses_scene" not in src and "WO_SKY_RAYS" not in src
        _rows_and_segments(r, p, ref, segs, what)
        sizes.append(wl.jit_code_object(src)[0])

    infos = _all_builds(monkeypatch, "csg32_nested", None, check,
                        builds=["", "-DWO_SKY_RAYS_BOUNCE_MIN=1", "-DWO_SKY_RAYS_BOUNCE_MIN=65"], width=96, height=54, spp=4,
                        max_depth=8, seed=7)
    assert len(set(sizes)) == 1, sizes
    assert len({(i["kind"], i["vgprs"], i["scratch_bytes"], i["lds_bytes"]) for i in infos}) == 1, infos
