"""GPU: the a-trous denoiser (wo_denoise_device, wo_renderer_render_denoised).  Every comparison is on
the raw bits of every pixel against the numpy restatement of the header (tests/denoise_support.py,
which tests/test_denoise.py pins to wo_denoise_host and to the oracle's frames).  Rows behind the
output and behind the scratch keep a sentinel; every buffer is sized from the API's own answers."""
import numpy as np
import pytest

import denoise_support as ds
import feature_support as fs
import test_gpu_rays as tgr
from csgrenderer_amd import wololo as wl

pytestmark = pytest.mark.gpu

W, H = 67, 45  # a multiple of no tile size (32 x 8, 32 x 16); several workgroups each way
FORMS = ("lds", "direct", "auto")
LEVELS = (1, 3, 8)  # steps 1 .. 4 have an LDS form; at 8 levels a forced `lds` falls back above step 4
EDGES = [(1, 1), (3, 2), (130, 1), (1, 130), (257, 9)]  # 257: one pixel past a tile column
GUARD_ROWS = 5


def _to_device(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32).reshape(-1, 4).copy()).cuda()


def _sentinel_rows(rows):
    import torch
    return torch.full((rows, 4), ds.SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")


class DeviceInput:
    """An input's planes on the device, with their host bytes to show they are not written."""

    def __init__(self, color, albedo, normal, ids):
        self.h, self.w = color.shape[:2]
        self.host = [color, albedo, normal, ids]
        self.dev = [None if a is None else _to_device(a) for a in self.host]

    def ptr(self, i, passed=True):
        return self.dev[i].data_ptr() if passed and self.dev[i] is not None else 0

    def unchanged(self):
        for a, d in zip(self.host, self.dev):
            if a is not None:
                assert d.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes(), "an input plane was written"


_DEV = {}


def _synthetic_on_device(w, h):
    if (w, h) not in _DEV:
        inp = ds.synthetic_shared(w, h)
        _DEV[(w, h)] = DeviceInput(inp["color"], inp["albedo"], inp["normal"], inp["ids"])
    return _DEV[(w, h)]


def _run(dp, di, passed=(True, True, True), stream=None, extra_scratch=0):
    """wo_denoise_device into sentinel-filled buffers; the frame (h, w, 4) float32.  Checks the guard
    rows behind the output and behind the scratch the call asked for, and the inputs."""
    import torch
    w, h = di.w, di.h
    need = wl.denoise_scratch_bytes(w, h, dp)
    assert need == (2 if dp.levels > 1 else 1) * w * h * 16
    out = _sentinel_rows(w * h + GUARD_ROWS * w)
    scratch = _sentinel_rows(need // 16 + GUARD_ROWS * w + extra_scratch)
    s = stream if stream is not None else torch.cuda.current_stream()
    wl.denoise_device(dp, w, h, di.ptr(0), di.ptr(1, passed[0]), di.ptr(2, passed[1]), di.ptr(3, passed[2]),
                      out.data_ptr(), scratch.data_ptr(), need + 16 * extra_scratch, s.cuda_stream)
    s.synchronize()
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[w * h:] == ds.SENTINEL).all(), "a row behind the output was written"
    assert (scratch[need // 16:].cpu().numpy().view(np.uint32) == ds.SENTINEL).all(), "a row behind the scratch was written"
    di.unchanged()
    return got[:w * h].reshape(h, w, 4).view(np.float32)


def _all_cases(w, h, levels, what):
    di = _synthetic_on_device(w, h)
    for name, fields, passed in ds.cases():
        exp, shares = ds.reference_shared(name, fields, passed, levels, w, h)
        dp = ds.case_params(fields, levels)
        if (w, h) == (W, H) and levels == 3:
            ds.check_shares(shares, dp, name)
        ds.same_bits(_run(dp, di, passed), exp, f"{what} {w}x{h} {name} levels {levels}")


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("form", FORMS)
def test_synthetic_frame_equals_the_reference(form, levels, monkeypatch):
    """67 x 45: each term alone, all together, both flags, NULL optional planes, in every form."""
    monkeypatch.setenv("WOLOLO_DENOISE_FORM", form)
    _all_cases(W, H, levels, form)


@pytest.mark.parametrize("w,h", EDGES)
@pytest.mark.parametrize("form", FORMS)
def test_edge_frames(form, w, h, monkeypatch):
    monkeypatch.setenv("WOLOLO_DENOISE_FORM", form)
    for levels in LEVELS:
        _all_cases(w, h, levels, form)


@pytest.mark.parametrize("form", FORMS)
def test_guards_streams_and_repeats(form, monkeypatch):
    """A side stream, two calls with identical bytes, and scratch larger than asked."""
    import torch
    monkeypatch.setenv("WOLOLO_DENOISE_FORM", form)
    di = _synthetic_on_device(W, H)
    name, fields, passed = ds.cases()[4]  # every term and both flags
    for levels in (1, 4):
        dp = ds.case_params(fields, levels)
        exp, _ = ds.reference_shared(name, fields, passed, levels, W, H)
        first = _run(dp, di, passed)
        ds.same_bits(first, exp, f"{form} levels {levels}")
        assert _run(dp, di, passed).tobytes() == first.tobytes()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        ds.same_bits(_run(dp, di, passed, stream=side), exp, f"{form} levels {levels} on a side stream")
        ds.same_bits(_run(dp, di, passed, extra_scratch=3 * W + 1), exp, f"{form} levels {levels}, larger scratch")


@pytest.mark.parametrize("scene", ["csg32", "rtiow_cover"])
def test_real_chain(scene, monkeypatch):
    """render_rows_device (rank 0 of 1) -> render_features_device -> wo_denoise_device, against the
    reference applied to the planes copied back; Renderer.render_denoised and wl.denoise_host give the
    same bytes; and the denoised frame is one the present encode takes (wo_srgb8_encode_device of it
    equals wo_srgb8_encode_host of the reference)."""
    import torch
    r = tgr._renderer(scene)
    p = fs.params(W, H, 3, seed=9, sample_offset=5)
    stream = torch.cuda.current_stream().cuda_stream
    rows = wl.local_rows(H, 16, 1)
    d_frame = torch.zeros((rows * W, 4), dtype=torch.float32, device="cuda")
    d_planes = torch.zeros((3 * H * W, 4), dtype=torch.int32, device="cuda")
    r.render_rows_device(p, d_frame.data_ptr(), 16, 0, 1, stream)
    r.render_features_device(p, d_planes.data_ptr(), H * W, H, 0, 1, stream)
    torch.cuda.synchronize()
    color = d_frame.cpu().numpy()[:H * W].reshape(H, W, 4)
    planes = d_planes.cpu().numpy().view(np.uint32).reshape(3, H, W, 4)
    albedo, normal = planes[0].view(np.float32), planes[1].view(np.float32)
    ids = planes[2].copy().view(ds.IDS_DT).reshape(H, W)
    assert np.isposinf(normal[..., 3]).any() and np.isfinite(normal[..., 3]).any()
    di = DeviceInput(color, albedo, normal, ids)
    for dp in (wl.denoise_params(), wl.denoise_params(levels=3, flags=wl.DENOISE_DEMODULATE | wl.DENOISE_STOP_AT_NODES)):
        exp, _ = ds.reference(dp, color, albedo, normal, ids)
        assert np.isfinite(exp).all() and (exp[..., :3] != color[..., :3]).any()
        for form in FORMS:
            monkeypatch.setenv("WOLOLO_DENOISE_FORM", form)
            ds.same_bits(_run(dp, di), exp, f"{scene} {form} levels {dp.levels}")
            ds.same_bits(r.render_denoised(p, dp), exp, f"{scene} {form} render_denoised")
        monkeypatch.delenv("WOLOLO_DENOISE_FORM")
        ds.same_bits(wl.denoise_host(dp, color, albedo, normal, ids), exp, f"{scene} host form")
    dp = wl.denoise_params()
    exp, _ = ds.reference(dp, color, albedo, normal, ids)
    ds.same_bits(r.render_denoised(p), exp, f"{scene} render_denoised with NULL parameters")
    # chaining: denoise -> present encode, all on the device
    need = wl.denoise_scratch_bytes(W, H, dp)
    d_out = torch.zeros((H * W, 4), dtype=torch.float32, device="cuda")
    d_scratch = torch.zeros(need // 4, dtype=torch.int32, device="cuda")
    d_bgra = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    wl.denoise_device(dp, W, H, di.ptr(0), di.ptr(1), di.ptr(2), di.ptr(3), d_out.data_ptr(), d_scratch.data_ptr(), need, stream)
    wl.srgb8_encode_device(d_out.data_ptr(), d_bgra.data_ptr(), H * W, stream)
    torch.cuda.synchronize()
    assert np.array_equal(d_bgra.cpu().numpy().view(np.uint32), wl.srgb8_encode_host(exp).reshape(-1))
    r.close()
