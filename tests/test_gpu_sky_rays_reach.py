"""GPU: the sky-ray predicate's level 4 (WO_SKY_RAYS=4: level 3 with each sphere member tested
by sphere_reaches, which also gives up a sphere whose far root is surely <= t_min -- the rays
that leave a sphere's own surface; scene_jit.c gen_sky_rays) changes neither the image nor the
segment count, wherever it runs.  Every frame below is bit-exact against the CPU oracle, with
the oracle's segment count, through render_rows_device, for the default build, level 3, and
level 4 in camera iterations only (the threshold's default), in every iteration (1) and from
24 lanes; the builds load different kernels, none uses scratch, and all have the same LDS.

The shapes are those of tests/test_gpu_sky_rays_terms.py, and one camera close to a sphere,
where most first hits lie on spheres: there level 4 ends rays that level 3 did not."""
import pytest

import test_gpu_sky_rays_bounce as tb
from csgrenderer_amd import wololo as wl

pytestmark = pytest.mark.gpu

BUILDS = ["", "-DWO_SKY_RAYS=3", "-DWO_SKY_RAYS=4", "-DWO_SKY_RAYS=4 -DWO_SKY_RAYS_BOUNCE_MIN=1",
          "-DWO_SKY_RAYS=4 -DWO_SKY_RAYS_BOUNCE_MIN=24"]
LDS = 17912  # the block's ring, sums, frame copy and records: no LDS of the predicate's
# 1.7 radii from the centre of the sphere at (0.42, 1.03, 3.65), r = 0.4: 97 % of the camera
# rays hit, 92 % of the first hits lie on a sphere (the host harness of tests/test_sky_rays.py)
AT_A_SPHERE = ((0.63, 1.37, 4.2), (0.42, 1.03, 3.65), (0, 1, 0), 50.0, 0.0, 10.0)


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


CAMERAS = dict(tb.CAMERAS, **{"at a sphere": AT_A_SPHERE})


@pytest.mark.parametrize("camera", list(CAMERAS), ids=[c.replace(" ", "_") for c in CAMERAS])
def test_csg32_cameras(camera, monkeypatch):
    """The cameras of the threshold's tests (floor up, inside group 1, inside the slab, all
    geometry behind, a lens), and one at a sphere: nearly every ray it scatters starts on a
    sphere's surface."""
    def check(r, p, ref, segs, what):
        tb._rows_and_segments(r, p, ref, segs, what)
        if camera == "behind":
            assert segs == p.width * p.height * p.spp
        else:
            assert segs > p.width * p.height * p.spp
    _resources(_all(monkeypatch, "csg32", CAMERAS[camera], check, width=96, height=54, spp=4, max_depth=8, seed=11))


def test_csg32_union(monkeypatch):
    infos = _all(monkeypatch, "csg32_union", None, tb._rows_and_segments, width=96, height=54, spp=4, max_depth=8, seed=7)
    _resources(infos, lds=infos[1]["lds_bytes"])
    assert infos[1]["lds_bytes"] >= LDS, infos  # (its own record and material counts)
