"""GPU: first-hit feature buffers (wo_renderer_render_features_device, wo_renderer_render_features).
Every comparison is on the raw bits of all three planes against the CPU reference
(tests/feature_support.py over tests/host/feature_ref.c, pinned to the oracle by
tests/test_features.py); no pixel is excluded.  Rows the call must not write keep a sentinel."""
import numpy as np
import pytest

import feature_support as fs
import test_gpu_rays as tgr
from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl

pytestmark = pytest.mark.gpu

W, H = 67, 45  # no multiple of 8 or 64; 16-row tiles leave three local rows past the frame
CASES = [(s, "interpreter") for s in ("csg32", "csg32_nested", "csg32_union", "rtiow_cover")] + \
    [(s, "lanes") for s in tgr.LANE_FORMS]
FOOTPRINTS = ("8x8", "64x1")  # query_launch.hip feature_tile


@pytest.fixture(scope="module")
def feature_lib(tmp_path_factory):
    return fs.build_feature_ref(tmp_path_factory.mktemp("feature_ref"))


_REFS = {}


def _reference(feature_lib, r, key, p):
    """The reference planes of frame p, made once per (scene, size, spp, ...) key and shared."""
    key = (key, p.width, p.height, p.spp, p.seed, p.sample_offset)
    if key not in _REFS:
        _REFS[key] = fs.FeatureScene(feature_lib, r).frame(p)
    return _REFS[key]


def _buffer(rows):
    import torch
    return torch.full((rows, 4), fs.SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")


def _words(buf):
    import torch
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint32)


def _device(r, p, tile_rows=16, rank=0, nranks=1, band=(0, 0), pad=0):
    """The device form on the current stream into a sentinel-filled buffer: uint32 (3 * stride, 4)."""
    import torch
    stride = wl.local_rows(p.height, tile_rows, nranks, band) * p.width + pad
    buf = _buffer(3 * stride)
    r.render_features_device(p, buf.data_ptr(), stride, tile_rows, rank, nranks, torch.cuda.current_stream().cuda_stream)
    return _words(buf)


def _check_path(r, scene, path):
    assert r.ray_path() == path
    if path == "lanes":
        assert r.lanes_info()["kind"] == tgr.LANE_FORMS[scene]
    else:
        info = r.lanes_info()
        assert info is None or info["kind"] not in tgr.LANE_FORMS.values()


@pytest.mark.parametrize("scene,path", CASES)
def test_planes_equal_the_reference(feature_lib, scene, path, monkeypatch):
    """67 x 45 at spp 1, 3 and 5, nonzero seed and sample_offset (rtiow_cover: through the lens):
    the device form, the host form, two workgroups (many trips of the grid-stride loop) and
    both footprints of a wave."""
    r = tgr._renderer(scene)
    r.set_ray_tracer(path)
    for spp in (1, 3, 5):
        p = fs.params(W, H, spp, seed=9, sample_offset=5)
        planes = _reference(feature_lib, r, scene, p)
        hits = planes[3]
        assert (hits == spp).any() and (hits == 0).any()
        exp = fs.rank_buffer(planes, p, 16, 0, 1)
        assert (exp[H * W:48 * W] == fs.SENTINEL).all()  # the three local rows past the frame
        fs.same_words(_device(r, p), exp, f"{scene} {path} spp {spp}")
        _check_path(r, scene, path)
        fs.same_planes(r.render_features(p), planes, f"{scene} {path} spp {spp} host form")
        _check_path(r, scene, path)
        if spp != 3:
            continue
        assert ((hits > 0) & (hits < spp)).any()
        for tile in FOOTPRINTS:
            monkeypatch.setenv("WOLOLO_FEATURE_TILE", tile)
            fs.same_words(_device(r, p), exp, f"{scene} {path} {tile}")
            monkeypatch.setenv("WOLOLO_RAY_BLOCKS", "2")
            fs.same_words(_device(r, p), exp, f"{scene} {path} {tile} two workgroups")
            monkeypatch.delenv("WOLOLO_RAY_BLOCKS")
        monkeypatch.delenv("WOLOLO_FEATURE_TILE")
    r.close()


@pytest.mark.parametrize("w,h", [(1, 1), (130, 1), (1, 130)])
@pytest.mark.parametrize("scene,path", [("csg32", "interpreter"), ("csg32_union", "lanes")])
def test_edge_frames(feature_lib, scene, path, w, h, monkeypatch):
    r = tgr._renderer(scene)
    r.set_ray_tracer(path)
    p = fs.params(w, h, 3, seed=4, sample_offset=2)
    planes = _reference(feature_lib, r, scene, p)
    exp = fs.rank_buffer(planes, p, 16, 0, 1)
    for tile in FOOTPRINTS:
        monkeypatch.setenv("WOLOLO_FEATURE_TILE", tile)
        fs.same_words(_device(r, p), exp, f"{scene} {path} {w}x{h} {tile}")
        monkeypatch.setenv("WOLOLO_RAY_BLOCKS", "2")
        fs.same_words(_device(r, p), exp, f"{scene} {path} {w}x{h} {tile} two workgroups")
        monkeypatch.delenv("WOLOLO_RAY_BLOCKS")
    _check_path(r, scene, path)
    fs.same_planes(r.render_features(p), planes, f"{scene} {path} {w}x{h} host form")
    r.close()


@pytest.mark.parametrize("band", [(0, 0), (2, 1)])
@pytest.mark.parametrize("scene,path", [("csg32_nested", "interpreter"), ("csg32_union", "lanes")])
def test_row_tiles_over_ranks(feature_lib, scene, path, band):
    """tile_rows = 4 over three ranks, plain and with weighted bands: every rank's buffer holds the
    reference's rows of that rank; and, written rank-major through plane_stride, each plane is a
    gathered frame that wo_assemble_rows_device_ex turns into the one-rank plane."""
    import torch
    r = tgr._renderer(scene)
    r.set_ray_tracer(path)
    if band != (0, 0):
        r.set_band_weight(*band)
    p = fs.params(W, H, 3, seed=9, sample_offset=5)
    planes = _reference(feature_lib, r, scene, p)
    tile_rows, nranks = 4, 3
    rows = wl.local_rows(H, tile_rows, nranks, band)
    assert rows == (16 if band == (0, 0) else 20)
    for rank in range(nranks):
        exp = fs.rank_buffer(planes, p, tile_rows, rank, nranks, band)
        fs.same_words(_device(r, p, tile_rows, rank, nranks, band), exp, f"{scene} {path} rank {rank} band {band}")
    _check_path(r, scene, path)
    # plane p of the gathered buffer: the ranks' local buffers one after another
    share, stream = rows * W, torch.cuda.current_stream().cuda_stream
    gathered = _buffer(3 * nranks * share)
    for rank in range(nranks):
        r.render_features_device(p, gathered.data_ptr() + 16 * rank * share, nranks * share, tile_rows, rank, nranks, stream)
    frame = _buffer(3 * H * W)
    for k in range(3):
        wl.assemble_rows_device(gathered.data_ptr() + 16 * k * nranks * share, frame.data_ptr() + 16 * k * H * W, W, H,
                                tile_rows, nranks, stream, band)
    got = _words(frame).reshape(3, H, W, 4)
    for k, name in enumerate(("albedo", "normal", "ids")):
        assert (got[k] == fs.as_words(planes[k])).all(), f"{scene} {path} band {band}: assembled {name} plane"
    r.close()


def test_padding_rows_keep_their_content(feature_lib):
    r = tgr._renderer("csg32")
    p = fs.params(W, H, 1, seed=9, sample_offset=5)
    planes = _reference(feature_lib, r, "csg32", p)
    exp = fs.rank_buffer(planes, p, 16, 0, 1, plane_stride=48 * W + 37)
    assert len(exp) == 3 * (48 * W + 37) and (exp[-37:] == fs.SENTINEL).all()
    fs.same_words(_device(r, p, pad=37), exp, "plane_stride 37 rows larger than needed")
    r.close()


def test_black_scene_albedo_is_the_frame(feature_lib):
    """csg32 with every leaf black, max_depth = 1: the frame is the mean sky of the samples that
    miss, and so is the albedo plane -- the feature rays are the rays the path kernels shoot,
    the interpreter's and the specialised kernel's."""
    import torch
    r = wl.Renderer("black", max_nodes=4096)
    scenes.build("csg32", r)
    fs.blacken(r)
    p = fs.params(W, H, 3, seed=9, sample_offset=5, max_depth=1)
    planes = _reference(feature_lib, r, "csg32 black", p)
    albedo = _device(r, p)[:H * W].reshape(H, W, 4)
    assert (albedo == fs.as_words(planes[0])).all() and r.ray_path() == "interpreter"
    hits = planes[3]
    assert (hits == 0).any() and (hits == 3).any() and ((hits > 0) & (hits < 3)).any()
    for tracer in ("interpreter", "jit"):
        r.set_tracer(tracer)
        frame = torch.zeros((48, W, 4), dtype=torch.float32, device="cuda")
        r.render_rows_device(p, frame.data_ptr(), 16, 0, 1, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert r.trace_path() == tracer
        got = frame.cpu().numpy()[:H].view(np.uint32)
        assert (got[..., :3] == albedo[..., :3]).all(), tracer
    r.close()


def test_ids_equal_pick(feature_lib):
    r = tgr._renderer("csg32_nested")
    p = fs.params(W, H, 2, seed=9, sample_offset=5)
    _, _, ids = r.render_features(p)
    rng = np.random.default_rng(16)
    xs, ys = rng.integers(0, W, size=16), rng.integers(0, H, size=16)
    picks = np.array([r.pick(p, x, y) for x, y in zip(xs, ys)], dtype=tgr.HIT_DT)
    assert 3 <= ((picks["flags"] & wl.RAY_HIT) != 0).sum() <= 15
    for name in ("node", "leaf", "material", "flags"):
        assert np.array_equal(ids[name][ys, xs], picks[name]), name
    r.close()


def test_empty_scene(feature_lib):
    r = wl.Renderer("empty", max_nodes=4)
    p = fs.params(W, H, 3, seed=9, sample_offset=5)
    planes = _reference(feature_lib, r, "empty", p)
    assert not planes[3].any()
    fs.same_words(_device(r, p), fs.rank_buffer(planes, p, 16, 0, 1), "empty scene")
    fs.same_planes(r.render_features(p), planes, "empty scene, host form")
    assert r.ray_path() == "interpreter"
    r.close()


def test_scene_edit_side_stream_and_repeats(feature_lib):
    """Two identical calls give identical bits; a call on a non-default stream is ordered after a
    fill of its buffer on that stream; a scene edit between two calls is seen by the second."""
    import torch
    r = wl.Renderer("edit", max_nodes=4096)
    scenes.build("csg32", r)
    p = fs.params(W, H, 3, seed=9, sample_offset=5)
    before = _reference(feature_lib, r, "csg32", p)
    exp0 = fs.rank_buffer(before, p, 16, 0, 1)
    first = _device(r, p)
    fs.same_words(first, exp0, "before the edit")
    assert _device(r, p).tobytes() == first.tobytes()
    side = torch.cuda.Stream()
    buf = torch.zeros((3 * 48 * W, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        buf.fill_(fs.SENTINEL - (1 << 32))
    r.render_features_device(p, buf.data_ptr(), 48 * W, 16, 0, 1, side.cuda_stream)
    side.synchronize()
    fs.same_words(buf.cpu().numpy().view(np.uint32), exp0, "behind a fill on a side stream")
    # a sphere in front of the camera (which looks from (0, 4.5, 10) at (0, 0.6, 0)), unioned in
    ball = r.sphere(0.8)
    r.union(wl.arg(ball, (0.0, 3.4, 7.2)), wl.arg(ball, (0.3, 3.4, 7.2)))
    after = _reference(feature_lib, r, "csg32 edited", p)
    on_ball = after[2]["node"] == ball
    assert on_ball.sum() >= 20 and (before[2]["node"] != ball).all()
    fs.same_words(_device(r, p), fs.rank_buffer(after, p, 16, 0, 1), "after the edit")
    fs.same_planes(r.render_features(p), after, "after the edit, host form")
    r.close()
