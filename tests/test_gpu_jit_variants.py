"""GPU parity of every compile-time variant of the specialised kernel: each row of
tests/jit_variants.py's table, at each of its frames, is the CPU oracle's image bit for bit
with the oracle's segment count, and the variant is the kernel that ran.

What each row is (that it compiles for gfx950, and that its machine code differs from the
default's on that scene) is settled on the CPU by tests/test_jit_variants.py; nothing here has
a tolerance.
"""
import pytest

import jit_variants as jv
import pyoracle
from csgrenderer_amd import wololo as wl
from test_gpu_parity import _check_path, _cmp, _oracle_rows
from test_jit_variants import frame_of, open_scene, row_id, rows, source_of, variant_flags

pytestmark = pytest.mark.gpu

MODES = [wl.MODE_NORMALS, wl.MODE_PATHTRACE]
RANK, NRANKS, RANK_TILE = 1, 3, 4
_REFS = {}
_KEYS = {}


def _ref(r, scene, frame, mode):
    """The oracle's frame and segment count of a scene's frame: computed once, shared, read-only."""
    what = (scene, "61x35" if frame == "rank1of3" else frame, mode)
    if what not in _REFS:
        img, segs = _oracle_rows(r, frame_of(scene, frame, mode))
        img.setflags(write=False)
        _REFS[what] = (img, segs)
    return _REFS[what]


def _rank_segments(r, scene, p):
    """The oracle's segments of the rows rank 1 of 3 renders in 4-row tiles, band by band."""
    if (scene, "rank") not in _REFS:
        prog, nrec, _ = r.program()
        mats, nm = r.materials()
        fr, segs = r.frame_desc(p), 0
        for lb in range(wl.rank_bands(p.height, RANK_TILE, RANK, NRANKS)):
            g0 = wl.band_global(lb, RANK, NRANKS) * RANK_TILE
            segs += pyoracle.pathtrace_rows(prog, nrec, mats, nm, fr, g0, min(RANK_TILE, p.height - g0))[1]
        _REFS[(scene, "rank")] = segs
    return _REFS[(scene, "rank")]


def _key(src, flags, arch, monkeypatch):
    """The key of (source, flags): what wo_jit_code_object builds under WOLOLO_JIT_FLAGS=flags."""
    if (src, flags) not in _KEYS:
        if flags:
            monkeypatch.setenv("WOLOLO_JIT_FLAGS", flags)
        else:
            monkeypatch.delenv("WOLOLO_JIT_FLAGS", raising=False)
        _KEYS[(src, flags)] = wl.jit_code_object(src, arch)[3]
    return _KEYS[(src, flags)]


def _rows_device(r, p, tile, rank, nranks):
    """(local rows as numpy, segment counter) of one render_rows_device call."""
    import torch

    lr = wl.local_rows(p.height, tile, nranks)
    out = torch.zeros((lr, p.width, 4), dtype=torch.float32, device="cuda")
    seg = torch.zeros(1, dtype=torch.int64, device="cuda")
    r.render_rows_device(p, out.data_ptr(), tile, rank, nranks, torch.cuda.current_stream().cuda_stream, seg.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(seg.item())


CASES = [row + (f,) for row in rows() for f in jv.TABLE[row[0]]["frames"]]


@pytest.mark.parametrize("case", CASES, ids=row_id)
def test_variant_is_bitexact_and_is_the_kernel_that_ran(case, monkeypatch):
    import torch

    macro, value, scene, extra, frame = case
    arch = torch.cuda.get_device_properties(0).gcnArchName
    src0 = source_of(scene, {}, monkeypatch)
    flags, base, env = variant_flags(macro, value, src0, extra, jv.TABLE[macro]["needs"])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if flags:
        monkeypatch.setenv("WOLOLO_JIT_FLAGS", flags)
    else:
        monkeypatch.delenv("WOLOLO_JIT_FLAGS", raising=False)
    r = open_scene(scene, "jit")
    what = row_id(case)
    if frame == "rank1of3":
        # the rank's rows come through the band map, and the tail writes local rows
        p = frame_of(scene, frame, wl.MODE_PATHTRACE)
        got, segs = _rows_device(r, p, RANK_TILE, RANK, NRANKS)
        _check_path(r, "jit", scene)
        ref, _ = _ref(r, scene, frame, wl.MODE_PATHTRACE)
        mine = wl.rank_bands(p.height, RANK_TILE, RANK, NRANKS) * RANK_TILE
        grow = [wl.global_row(lr, RANK_TILE, RANK, NRANKS) for lr in range(mine)]
        keep = [lr for lr, g in enumerate(grow) if g < p.height]
        assert len(keep) == 3 * RANK_TILE  # bands 1, 4 and 7 of the frame's 9
        _cmp(got[keep], ref[[grow[lr] for lr in keep]], what)
        assert segs == _rank_segments(r, scene, p), what
    else:
        for mode in MODES:
            p = frame_of(scene, frame, mode)
            img = r.render(p)
            _check_path(r, "jit", scene)
            ref, want = _ref(r, scene, frame, mode)
            _cmp(img, ref, f"{what} mode={mode}")
        got, segs = _rows_device(r, p, 8, 0, 1)  # (path trace: the last mode)
        _cmp(got[:p.height], ref, f"{what} rows")
        assert segs == want, what
    src = r.jit_source()
    k = r.kernel_info()
    r.close()
    for name in env:
        monkeypatch.delenv(name)
    # the variant is the kernel that ran: the key of its (source, flags), not the default's
    assert (src != src0) == bool(env), what
    assert k["key"] == _key(src, flags, arch, monkeypatch), what
    assert k["key"] != _key(src0, base, arch, monkeypatch), what
