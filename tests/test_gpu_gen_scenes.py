"""GPU parity on the generated scenes of tests/test_gen_scenes.py: every row of its case
table on every tracer, bit for bit against the CPU oracle.

The named scenes of test_gpu_parity.py pin one branch each of the choices scene_jit.c and
lane_bvh_build.cpp make from the structure of the tree; the rows here reach the others
(flat root evaluation, decision lists beside truth tables, levelled tables with their words
in registers, term mode over two membership words, the program in global memory, RDIFF
records, coincident surfaces ...).  What each row is for is asserted on the CPU
(test_gen_scenes.py) and again here on the source actually rendered.  The ray queries meet
a reference that shares no code with the oracle: the float64 point classifier.
"""
import pytest

import gen_scenes as gs
from csgrenderer_amd import wololo as wl
from test_gen_scenes import (BY_NAME, CASES, H, NAMES, W, check_facts, frame_params, hits_vs_classifier, make,
                             ray_batch)
from test_gpu_parity import PATHS, _check_path, _cmp, _oracle_rows
from test_gpu_rays import _same

pytestmark = pytest.mark.gpu

MODES = [wl.MODE_NORMALS, wl.MODE_PATHTRACE]
_REFS = {}


def _ref(r, name, mode):
    """The oracle's frame and segment count of a row: computed once, shared, read-only."""
    if (name, mode) not in _REFS:
        img, segs = _oracle_rows(r, frame_params(mode))
        img.setflags(write=False)
        _REFS[(name, mode)] = (img, segs)
    return _REFS[(name, mode)]


def _rendered_facts(r):
    """check_facts' source-side facts, from the source of the kernel that rendered."""
    src = r.jit_source()
    d = gs.describe(r)
    d["forms"] = gs.forms(src)
    return d


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", NAMES)
def test_frames_bitexact(name, path):
    case = BY_NAME[name]
    r, _ = make(case, path)
    for mode in MODES:
        img = r.render(frame_params(mode))
        _check_path(r, path, name)
        ref, _ = _ref(r, name, mode)
        _cmp(img, ref, f"{name} mode={mode} path={path}")
    if path == "jit":
        check_facts(case, _rendered_facts(r))
    if path == "lanes":
        assert r.lanes_info()["kind"] == case.want["lane"]["kind"], r.lanes_info()
    r.close()


@pytest.mark.parametrize("name", NAMES)
def test_segment_count(name):
    """One tracer per row (they take turns) through render_rows_device with a segment
    counter: the oracle's count, and the same frame."""
    import torch

    case = BY_NAME[name]
    path = PATHS[NAMES.index(name) % len(PATHS)]
    r, _ = make(case, path)
    p = frame_params(wl.MODE_PATHTRACE)
    tile = 8
    rows = wl.local_rows(H, tile, 1)
    assert rows >= H
    out = torch.zeros((rows, W, 4), dtype=torch.float32, device="cuda")
    seg = torch.zeros(1, dtype=torch.int64, device="cuda")
    r.render_rows_device(p, out.data_ptr(), tile, 0, 1, torch.cuda.current_stream().cuda_stream, seg.data_ptr())
    torch.cuda.synchronize()
    _check_path(r, path, name)
    ref, segs = _ref(r, name, wl.MODE_PATHTRACE)
    assert int(seg.item()) == segs, (name, path)
    _cmp(out[:H].cpu().numpy(), ref, f"{name} rows path={path}")
    r.close()


def _rows_with(form):
    return [c.name for c in CASES if form in c.want["forms"]]


LDS_EVENTS = "-DWO_JIT_LDS_EVENTS=1"
# compile-time variants of the generated source (all #ifndef-guarded there): they change how a
# wave works, never the image.  Every list comes from the table: a new row of a form joins it.
VARIANTS = (
    # the flat evaluation of a tree that defaults to truth tables
    [(n, "-DWO_JIT_LUT=0") for n in _rows_with("lut")]
    # the levelled tables' membership words in registers and in LDS, whichever the row defaults to
    + [(n, f"-DWO_HBITS_LDS={v}") for n in _rows_with("hlut") for v in (0, 1)]
    # term mode over two words without the per-tile pre-cull
    + [("term_64", "-DWO_CAM_TILE_CULL=0")]
    # the LDS event list under the flat evaluation and under ties, at its default size and at 2
    + [(n, f) for n in _rows_with("flat") + ["ties_nest"] for f in (LDS_EVENTS, LDS_EVENTS + " -DWO_LDS_EVENTS=2")]
    # a register window of 2 events on a general tree: overflow and re-collect
    + [("flat_w2", "-DWO_WINDOW=2")])


def _resources(src, arch, flags, monkeypatch):
    """(scratch, LDS) bytes and key of the source's code object under WOLOLO_JIT_FLAGS=flags."""
    if flags:
        monkeypatch.setenv("WOLOLO_JIT_FLAGS", flags)
    else:
        monkeypatch.delenv("WOLOLO_JIT_FLAGS", raising=False)
    return wl.jit_code_resources(src, arch), wl.jit_code_object(src, arch)[3]


@pytest.mark.parametrize("name,flags", VARIANTS)
def test_compile_flag_variants(name, flags, monkeypatch):
    """The image is the oracle's under every variant, and the variant is the kernel that ran:
    the source text does not change with a flag (its defaults sit under #ifndef), so the
    loaded code object is told from the default one by its key and by the static LDS its
    kernel descriptor states -- the event list, the truth tables, the membership words and
    the tile pre-cull's words all live there, so a flag that did not reach the compiler, or
    a misspelt one, leaves the LDS bytes at the default's."""
    import torch

    arch = torch.cuda.get_device_properties(0).gcnArchName
    case = BY_NAME[name]
    monkeypatch.setenv("WOLOLO_JIT_FLAGS", flags)
    r, _ = make(case, "jit")
    for mode in MODES:
        img = r.render(frame_params(mode))
        _check_path(r, "jit", name)
        ref, _ = _ref(r, name, mode)
        _cmp(img, ref, f"{name} {flags} mode={mode}")
    src = r.jit_source()
    assert gs.forms(src) == case.want["forms"]
    k = r.kernel_info()
    r.close()
    (scratch0, lds0), key0 = _resources(src, arch, "", monkeypatch)
    print(name, flags, "LDS", k["lds_bytes"], "default", lds0)
    assert k["key"] != key0 and k["key"] == _resources(src, arch, flags, monkeypatch)[1]
    if "WO_JIT_LUT=0" in flags or "WO_CAM_TILE_CULL=0" in flags:
        assert k["lds_bytes"] < lds0  # no tables / no pre-cull words in LDS
    elif "WO_HBITS_LDS" in flags:
        default = gs.define(src, "WO_HBITS_LDS")
        want = int(flags[-1])
        if want == default:
            assert (k["scratch_bytes"], k["lds_bytes"]) == (scratch0, lds0)
        else:
            assert (k["lds_bytes"] > lds0) == (want == 1) and k["lds_bytes"] != lds0
    elif "WO_LDS_EVENTS=2" in flags:
        (_, lds_full), _ = _resources(src, arch, LDS_EVENTS, monkeypatch)
        assert lds0 < k["lds_bytes"] < lds_full  # a list, and a shorter one than the default
    elif LDS_EVENTS in flags:
        assert k["lds_bytes"] > lds0
    # (WO_WINDOW=2 changes registers, not LDS: test_recollects_happen pins it)


@pytest.mark.parametrize("name,flags", [("flat_w2", "-DWO_WINDOW=2"), ("ties_nest", "")])
def test_recollects_happen(name, flags, monkeypatch):
    """The overflow path is the one tested: the counting variant of the row's kernel reports
    re-collects, and traces the oracle's segments."""
    if flags:
        monkeypatch.setenv("WOLOLO_JIT_FLAGS", flags)
    case = BY_NAME[name]
    r, _ = make(case, "jit")
    p = frame_params(wl.MODE_PATHTRACE)
    r.render(p)
    _check_path(r, "jit", name)
    w = r.count_work(p, 8, 0, 1)
    print(name, flags, {k: w[k] for k in ("segments", "recollects", "events", "sweep_steps")})
    assert w["segments"] == _ref(r, name, wl.MODE_PATHTRACE)[1]
    assert w["recollects"] > 0
    r.close()


def _ray_cases():
    out = []
    for c in CASES:
        out.append((c.name, "interpreter"))
        if c.want["lane"]["union_only"]:
            out.append((c.name, "lanes"))
    return out


@pytest.mark.parametrize("name,path", _ray_cases())
def test_rays_bitexact_and_against_the_classifier(name, path):
    """About 1 000 seeded rays per row (test_gpu_rays.make_batch's groups): the device's rows
    are the oracle's as bits, and -- rows without coincident surfaces -- every hit lies where
    the float64 classifier changes membership, RAY_ENTERS its membership behind the hit."""
    case = BY_NAME[name]
    r, sh = make(case, "interpreter")
    _, rays, exp = ray_batch(r, case)
    r.set_ray_tracer(path)
    got = r.trace_rays(rays)
    assert r.ray_path() == path
    if path == "lanes":
        assert r.lanes_info()["kind"] == case.want["lane"]["kind"], r.lanes_info()
    _same(got, exp, f"{name} {path}")
    if not case.want.get("ties"):
        hits_vs_classifier(sh, rays, got, f"{name} {path} (device)")
    r.close()
