"""GPU: the sky-ray predicate's level 3 (WO_SKY_RAYS=3: every group opened down to its terms,
each term's first literal tested by one member -- its sphere, or the face pair of its box's
thinnest axis; scene_jit.c gen_sky_rays) changes neither the image nor the segment count,
wherever it runs.  Every frame below is bit-exact against the CPU oracle, with the oracle's
segment count, through render_rows_device, for the default build, level 2, and level 3 in
camera iterations only (the threshold's default), in every iteration (1) and from 24 lanes;
the builds load different kernels, none uses scratch, and all have the same LDS.

The shapes are those of tests/test_gpu_sky_rays_bounce.py: the smallest at which the loop's
control flow can go wrong."""
import pytest

import test_gpu_sky_rays_bounce as tb
from csgrenderer_amd import wololo as wl

pytestmark = pytest.mark.gpu

BUILDS = ["", "-DWO_SKY_RAYS=2", "-DWO_SKY_RAYS=3", "-DWO_SKY_RAYS=3 -DWO_SKY_RAYS_BOUNCE_MIN=1",
          "-DWO_SKY_RAYS=3 -DWO_SKY_RAYS_BOUNCE_MIN=24"]
LDS = 17912  # the block's ring, sums, frame copy and records: no LDS of the predicate's


def _all(monkeypatch, scene, camera, check, **over):
    return tb._all_builds(monkeypatch, scene, camera, check, builds=BUILDS, **over)


def _resources(infos, lds=LDS):
    """Five builds: five kernels (the default's key differs from an explicit level's by its
    options), none with scratch, the LDS of the kernel as it was."""
    assert len({i["key"] for i in infos}) == len(infos) == len(BUILDS), infos
    assert [i["scratch_bytes"] for i in infos] == [0] * len(BUILDS), infos
    assert [i["lds_bytes"] for i in infos] == [lds] * len(BUILDS), infos


@pytest.mark.parametrize("spp", [1, 3, 5, 8])
def test_csg32_own_camera_spp(spp, monkeypatch):
    _resources(_all(monkeypatch, "csg32", None, tb._rows_and_segments, width=96, height=54, spp=spp, max_depth=8, seed=11))


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_csg32_depths(depth, monkeypatch):
    def check(r, p, ref, segs, what):
        tb._rows_and_segments(r, p, ref, segs, what)
        if depth == 1:
            assert segs == p.width * p.height * p.spp
        else:
            assert segs > p.width * p.height * p.spp
    _resources(_all(monkeypatch, "csg32", None, check, width=96, height=54, spp=4, max_depth=depth, seed=7))


@pytest.mark.parametrize("spp", [1, 130, 400])
def test_csg32_single_pixel(spp, monkeypatch):
    _resources(_all(monkeypatch, "csg32", None, tb._rows_and_segments, width=1, height=1, spp=spp, max_depth=8, seed=3))


@pytest.mark.parametrize("w,h", [(13, 7), (61, 35)])
def test_csg32_partial_tiles(w, h, monkeypatch):
    _resources(_all(monkeypatch, "csg32", None, tb._rows_and_segments, width=w, height=h, spp=5, max_depth=8, seed=3))


def test_csg32_normals(monkeypatch):
    _resources(_all(monkeypatch, "csg32", None, tb._rows_and_segments, width=96, height=54, spp=1, max_depth=8,
                    mode=wl.MODE_NORMALS, seed=7))


@pytest.mark.parametrize("camera", list(tb.CAMERAS), ids=[c.replace(" ", "_") for c in tb.CAMERAS])
def test_csg32_cameras(camera, monkeypatch):
    """Floor up: nearly every continuing ray is ended by the test; in group 1 and in the slab:
    origins inside the bounds, and inside the slab's y extent, where the face pair accepts
    nothing; behind: nothing scatters; a lens."""
    def check(r, p, ref, segs, what):
        tb._rows_and_segments(r, p, ref, segs, what)
        if camera == "behind":
            assert segs == p.width * p.height * p.spp
        else:
            assert segs > p.width * p.height * p.spp
    _resources(_all(monkeypatch, "csg32", tb.CAMERAS[camera], check, width=96, height=54, spp=4, max_depth=8, seed=11))


def test_csg32_union(monkeypatch):
    """The slab as a one-literal term: the same face pair."""
    infos = _all(monkeypatch, "csg32_union", None, tb._rows_and_segments, width=96, height=54, spp=4, max_depth=8, seed=7)
    _resources(infos, lds=infos[1]["lds_bytes"])
    assert infos[1]["lds_bytes"] >= LDS, infos  # (its own record and material counts)


def test_three_ranks_four_row_tiles(monkeypatch):
    """3 ranks' 4-row tiles at 61x35, assembled: the one-rank frame, which is the oracle's."""
    import numpy as np
    import torch

    def check(r, p, ref, segs, what):
        full = r.render(p)
        tb._same(full, ref, what)
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
        assert int(seg.item()) == segs, what

    _resources(_all(monkeypatch, "csg32", None, check, width=61, height=35, spp=3, max_depth=8, seed=5))


def test_progressive_accumulation(monkeypatch):
    """Two accumulated launches of 4 spp == one render of 8 spp, from a non-zero sample offset;
    the frame itself through render_rows_device with its segment count."""
    def check(r, p, ref, segs, what):
        half = wl.render_params(p.width, p.height, spp=4, max_depth=p.max_depth, seed=p.seed, mode=p.mode,
                                sample_offset=p.sample_offset)
        img, n = r.render_accumulate(half, reset=True)
        assert n == 4
        img, n = r.render_accumulate(half)
        assert n == 8
        tb._same(img, ref, what + " 2 x 4 spp")
        tb._rows_and_segments(r, p, ref, segs, what)

    _resources(_all(monkeypatch, "csg32", None, check, width=61, height=35, spp=8, max_depth=8, seed=9, sample_offset=5))
