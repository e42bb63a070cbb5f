"""First-hit feature buffers, the host side (CPU only): the Wo_FeatureIds layout, the argument
checks (which come before the device is touched), and the CPU reference
(tests/host/feature_ref.c) pinned independently: its rays and RNG to the oracle's own frames, its
ids to the oracle's trace of wo_renderer_pixel_ray, and its sums to closed forms."""
import ctypes
import math

import numpy as np
import pytest

import feature_support as fs
import pyoracle
import test_gpu_rays as tgr
from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl

W, H = 48, 27


@pytest.fixture(scope="module")
def feature_lib(tmp_path_factory):
    return fs.build_feature_ref(tmp_path_factory.mktemp("feature_ref"))


def test_feature_ids_abi_and_symbols():
    assert ctypes.sizeof(wl.FeatureIds) == 16 and wl.abi_layout("Wo_FeatureIds") == 16
    dt = np.dtype(wl.FEATURE_IDS_FIELDS)
    assert dt.itemsize == 16
    assert [n for n, _ in wl.FeatureIds._fields_] == ["node", "leaf", "material", "flags"] == list(dt.names)
    for fname, _ in wl.FeatureIds._fields_:
        assert wl.abi_layout("Wo_FeatureIds", fname) == getattr(wl.FeatureIds, fname).offset == dt.fields[fname][1]
    lib = wl.load()
    for sym in ("wo_renderer_render_features_device", "wo_renderer_render_features"):
        assert hasattr(lib, sym) and sym in wl.SIGNATURES
    assert (wl.FEATURE_ALBEDO, wl.FEATURE_NORMAL, wl.FEATURE_IDS, wl.FEATURE_PLANES) == (0, 1, 2, 3)


def _pt(**kw):
    p = fs.params(W, H, 3)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_bad_arguments_are_named_without_a_device(hostonly):
    r = wl.Renderer("nodev", max_nodes=4)
    r.sphere(1.0)
    rows = wl.local_rows(H, 4, 3)
    stride, buf = rows * W, 0x10000  # never dereferenced: no device
    good = (_pt(), buf, stride, 4, 1, 3)
    cases = [
        ((None,) + good[1:], "NULL params"),
        ((_pt(width=0),) + good[1:], "width"),
        ((_pt(height=0),) + good[1:], "height"),
        ((_pt(spp=0),) + good[1:], "spp"),
        ((_pt(mode=wl.MODE_NORMALS),) + good[1:], "PATHTRACE"),
        ((_pt(mode=wl.MODE_UBERSHADER_RT1),) + good[1:], "PATHTRACE"),
        (good[:3] + (4, 0, 0), "nranks=0"),
        (good[:3] + (4, 3, 3), "rank=3"),
        (good[:3] + (4, 7, 3), "rank=7"),
        (good[:3] + (0, 1, 3), "tile_rows=0"),
        (good[:2] + (stride - 1,) + good[3:], "plane_stride"),
        (good[:2] + (0,) + good[3:], "plane_stride"),
        (good[:1] + (0,) + good[2:], "buffer"),
        (good[:1] + (buf + 8,) + good[2:], "aligned"),
        (good, "device"),  # valid arguments: the renderer has no device
    ]
    for args, word in cases:
        wl.clear_error()
        with pytest.raises(wl.WololoError, match=word):
            r.render_features_device(*args)
    # a weighted band changes the rank's rows, and with them the shortest stride
    r.set_band_weight(2, 1)
    rows_p, rows_w = wl.local_rows(45, 4, 3), wl.local_rows(45, 4, 3, (2, 1))
    assert (rows_p, rows_w) == (16, 20)
    wl.clear_error()
    with pytest.raises(wl.WololoError, match="plane_stride"):
        r.render_features_device(_pt(height=45), buf, rows_p * W, 4, 1, 3)
    wl.clear_error()
    with pytest.raises(wl.WololoError, match="device"):
        r.render_features_device(_pt(height=45), buf, rows_w * W, 4, 1, 3)
    # the host form
    lib, out = r.lib, np.zeros((3 * H * W + 1, 4), dtype=np.float32)
    assert out.ctypes.data % 16 == 0
    host = [(None, out.ctypes.data, "NULL params"), (_pt(width=0), out.ctypes.data, "width"),
            (_pt(spp=0), out.ctypes.data, "spp"), (_pt(mode=wl.MODE_NORMALS), out.ctypes.data, "PATHTRACE"),
            (_pt(), 0, "buffer"), (_pt(), out.ctypes.data + 4, "aligned"), (_pt(), out.ctypes.data, "device")]
    for p, addr, word in host:
        wl.clear_error()
        rc = lib.wo_renderer_render_features(r.ptr, ctypes.byref(p) if p is not None else None, ctypes.c_void_p(addr))
        assert rc == -1 and word in wl.last_error(), (word, wl.last_error())
    wl.clear_error()
    with pytest.raises(wl.WololoError, match="device"):
        r.render_features(_pt())
    assert not out.any() and r.ray_path() == "none"
    r.close()


@pytest.mark.parametrize("scene", ["csg32", "rtiow_cover"])
def test_reference_rays_are_the_oracles(feature_lib, hostonly, scene):
    """With every leaf black and max_depth = 1 a PATHTRACE pixel of the oracle is the mean of the
    sky over the samples that miss (a hit leaves the radiance 0), which is what the albedo plane
    holds then: the reference's RNG, jitter, lens and rays are the oracle's, bit for bit."""
    r = wl.Renderer(scene, max_nodes=4096)
    scenes.build(scene, r)
    fs.blacken(r)
    sc = fs.FeatureScene(feature_lib, r)
    p = fs.params(W, H, 3, seed=9, sample_offset=5, max_depth=1)
    fr = r.frame_desc(p)
    assert (fr.cam.lens_radius > 0) == (scene == "rtiow_cover")
    albedo, normal, ids, hits = sc.frame(p)
    frame, _ = pyoracle.pathtrace_rows(sc.prog, sc.nrec, sc.mats, sc.n_mats, fr, 0, H)
    assert 0.2 < (hits > 0).mean() and (hits == 0).any() and ((hits > 0) & (hits < 3)).any()
    assert albedo[..., :3].tobytes() == np.ascontiguousarray(frame[..., :3]).tobytes()
    assert np.array_equal(albedo[..., 3], (hits.astype(np.float64) / 3.0).astype(np.float32))
    assert (albedo[hits == 3][:, :3] == 0).all()
    r.close()


def test_reference_ids_are_the_oracles_trace_of_the_pixel_ray(feature_lib, hostonly):
    r = wl.Renderer("csg32_nested", max_nodes=4096)
    scenes.build("csg32_nested", r)
    sc = fs.FeatureScene(feature_lib, r)
    p = fs.params(W, H, 1)
    _, _, ids, _ = sc.frame(p)
    rays = np.stack([r.pixel_ray(p, x, y) for y in range(H) for x in range(W)])
    exp = tgr.Scene(r).expect(rays).reshape(H, W)
    for name in ("node", "leaf", "material", "flags"):
        assert np.array_equal(ids[name], exp[name]), name
    hit = ids["flags"] != 0
    assert 0.2 < hit.mean() < 0.95 and (ids["node"][~hit] == wl.WO_NODE_INVALID).all()
    assert len(np.unique(ids["node"][hit])) >= 8
    # the ids do not depend on spp, seed or sample_offset
    _, _, again, _ = sc.frame(fs.params(W, H, 2, seed=77, sample_offset=1000))
    assert again.tobytes() == ids.tobytes()
    r.close()


def _q(v):
    """oracle.c quantize_radiance of a float32."""
    v = float(np.float32(v))
    return int(v * 4294967296.0) if abs(v) < 1048576.0 else 0


def _m(total, n):
    """oracle.c mean_radiance."""
    return np.float32((float(total) * (1.0 / 4294967296.0)) / float(n))


def test_halfspace_closed_form(feature_lib, hostonly):
    """A lone half-space y <= 0 seen from above fills the frame: every sample hits it."""
    r = wl.Renderer("halfspace", max_nodes=4)
    plane = r.halfspace((0.0, 1.0, 0.0))
    mat = r.lambertian((0.25, 0.5, 0.75))
    r.set_material(plane, mat)
    r.set_camera((0.0, 5.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 40.0, 0.0, 5.0)
    sc = fs.FeatureScene(feature_lib, r)
    for spp in (1, 3, 5):
        albedo, normal, ids, hits = sc.frame(fs.params(W, H, spp))
        assert (hits == spp).all() and (albedo[..., 3] == 1.0).all()
        assert (normal[..., :3] == np.array([0.0, 1.0, 0.0], dtype=np.float32)).all()
        want = [_m(spp * _q(a), spp) for a in (0.25, 0.5, 0.75)]
        assert want == [0.25, 0.5, 0.75] and (albedo[..., :3] == np.array(want, dtype=np.float32)).all()
        assert (ids["node"] == plane).all() and (ids["flags"] == (wl.RAY_HIT | wl.RAY_ENTERS)).all()
        assert (ids["material"] == mat).all() and (sc.nodes[ids["leaf"]] == plane).all()
        depth = normal[..., 3]
        assert (depth >= 5.0 - 1e-5).all() and (depth < 5.0 / math.cos(math.radians(40.0))).all()
    r.close()


def test_empty_scene(feature_lib, hostonly):
    r = wl.Renderer("empty", max_nodes=4)
    sc = fs.FeatureScene(feature_lib, r)
    p = fs.params(W, H, 3, max_depth=1)
    albedo, normal, ids, hits = sc.frame(p)
    assert not hits.any() and not albedo[..., 3].any() and not normal[..., :3].any()
    assert np.isposinf(normal[..., 3]).all()
    assert (fs.as_words(ids) == np.array(fs.MISS_IDS, dtype=np.uint32)).all()
    frame, _ = pyoracle.pathtrace_rows(sc.prog, sc.nrec, sc.mats, sc.n_mats, r.frame_desc(p), 0, H)
    assert albedo[..., :3].tobytes() == np.ascontiguousarray(frame[..., :3]).tobytes()
    r.close()


def test_lone_sphere_depth_bounds(feature_lib, hostonly):
    """A sphere of radius rad at distance D: a first hit lies between the nearest point (D - rad)
    and the tangent points (sqrt(D^2 - rad^2)); 1e-4 D of slack is orders above fp32 error."""
    rad, D = 1.0, 6.0
    r = wl.Renderer("sphere", max_nodes=4)
    ball = r.sphere(rad)
    r.set_camera((0.0, 0.0, D), (0.0, 0.0, 0.0), (0, 1, 0), 30.0, 0.0, D)
    sc = fs.FeatureScene(feature_lib, r)
    albedo, normal, ids, hits = sc.frame(fs.params(W, H, 4))
    full = albedo[..., 3] == 1.0
    assert np.array_equal(full, hits == 4) and 50 <= full.sum() <= W * H - 200
    assert ((hits > 0) & (hits < 4)).any()
    depth = normal[..., 3][full]
    assert (depth >= D - rad - 1e-4 * D).all() and (depth <= math.sqrt(D * D - rad * rad) + 1e-4 * D).all()
    assert depth.min() < D - rad + 0.01 and depth.max() > D - rad + 0.05
    assert np.isposinf(normal[..., 3][hits == 0]).all() and (ids["node"][full] == ball).all()
    # a facing normal on a sphere seen from outside points at the camera's side
    assert (normal[..., 2][full] > 0).all()
    r.close()
