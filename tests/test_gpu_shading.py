"""GPU: the physics scenes of tests/physics_scenes.py on every tracer.

  a. bit-exact parity with the CPU oracle at 4096 spp and at the depth limits 1, 2, 3, 4, 8 and
     50 (the other parity files stop at a few spp and never use depth 1, 2, 3 or 50), once with
     a sample index that wraps past 2^32, segment counts equal;
  b. convergence on the closed forms at 2^18 spp, a count only the device can afford: the one
     check of the 32.32 fixed-point sum and of the random streams at a quarter of a million
     samples per pixel, eight times as tight as the CPU test (tests/test_shading_ref.py);
  c. csg32 at 16 x 12 and 2^16 spp, with and without the sky-ray and sky-tile kernel forms,
     against the float64 reference per 4 x 4 block, the builds byte-identical to each other.
"""
import contextlib

import numpy as np
import pytest

import physics_scenes as ps
import pyoracle
from csgrenderer_amd import wololo as wl
from test_shading_ref import Z_ACCEPT, reference

pytestmark = pytest.mark.gpu

PARITY_SPP = 4096
CONVERGENCE_SPP = 1 << 18
CSG32_SPP = 1 << 16
QUADRATURE_K = 32  # q falls with K^2: under 1e-5, below the standard errors at 2^18 spp

_oracle = {}
_closed = {}


def tracers(name):
    return ("jit", "interpreter", "lanes") if name in ps.UNION_ONLY else ("jit", "interpreter")


@contextlib.contextmanager
def renderer(name, tracer):
    rec = ps.make(name)
    try:
        rec.r.set_tracer(tracer)
        yield rec
    finally:
        rec.close()


def params(depth, spp, seed=5, sample_offset=0):
    return wl.render_params(ps.W, ps.H, spp=spp, max_depth=depth, seed=seed, mode=wl.MODE_PATHTRACE,
                            sample_offset=sample_offset)


def oracle(rec, name, p):
    key = (name, p.max_depth, p.spp, p.sample_offset)
    if key not in _oracle:
        prog, nrec, _ = rec.r.program()
        mats, nm = rec.r.materials()
        _oracle[key] = pyoracle.pathtrace_rows(prog, nrec, mats, nm, rec.r.frame_desc(p), 0, p.height)
    return _oracle[key]


def same(gpu, ref, what):
    """test_gpu_parity._cmp's bar: bit-exact."""
    gpu, ref = np.asarray(gpu, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert gpu.shape == ref.shape, what
    d = np.where(np.isnan(gpu) & np.isnan(ref), 0.0, np.abs(gpu.astype(np.float64) - ref.astype(np.float64)))
    nbad = int((d > 0).sum())
    assert nbad == 0, f"{what}: not bit-exact ({nbad} values differ, max {float(d.max())})"


def rows_and_segments(r, p):
    import torch
    out = torch.zeros((p.height, p.width, 4), dtype=torch.float32, device="cuda")
    seg = torch.zeros(1, dtype=torch.int64, device="cuda")
    r.render_rows_device(p, out.data_ptr(), 16, 0, 1, torch.cuda.current_stream().cuda_stream, seg.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(seg.item())


# ---- a. parity -----------------------------------------------------------------------------------
PARITY = [(name, depth, t) for name, depth in ps.CASES for t in tracers(name)]


@pytest.mark.parametrize("name,depth,tracer", PARITY)
def test_parity_at_4096_spp(name, depth, tracer):
    with renderer(name, tracer) as rec:
        p = params(depth, PARITY_SPP)
        ref, segs = oracle(rec, name, p)
        img, got = rows_and_segments(rec.r, p)
        assert rec.r.trace_path() == tracer
    same(img, ref, f"{name} depth {depth} {tracer}")
    assert got == segs, (name, depth, tracer, got, segs)


@pytest.mark.parametrize("tracer", tracers("ground_ball"))
def test_parity_when_the_sample_index_wraps(tracer):
    """Samples 0xFFFFF000 .. 0xFFFFFFFF, then 0 .. 0xFFF: 8192 spp from offset 2^32 - 4096."""
    with renderer("ground_ball", tracer) as rec:
        p = params(8, 2 * PARITY_SPP, sample_offset=0xFFFFF000)
        ref, segs = oracle(rec, "ground_ball", p)
        img, got = rows_and_segments(rec.r, p)
        assert rec.r.trace_path() == tracer
    same(img, ref, f"ground_ball wrapped {tracer}")
    assert got == segs, (tracer, got, segs)


# ---- b. convergence ------------------------------------------------------------------------------
def closed_form(name, depth):
    """(mean, per-sample variance, valid cells, q).  The variance is the closed form's where a
    sample's outcomes given its direction are discrete (mirror, slab, pool); the Lambertian lobe
    is continuous, so there it is the float64 reference's at its CPU sample count."""
    key = (name, depth)
    if key not in _closed:
        mean, var, valid, _ = ps.closed_form(name, depth, QUADRATURE_K)
        q = ps.quadrature_error(name, depth, QUADRATURE_K)
        if name == "lambert_sphere":
            var = reference(name, depth)[1]
        _closed[key] = (mean, var, valid, q)
    return _closed[key]


CONVERGENCE = [(name, depth, t) for name, depth in ps.CASES if name in ps.CLOSED_FORM for t in tracers(name)]


@pytest.mark.parametrize("name,depth,tracer", CONVERGENCE)
def test_convergence_on_the_closed_form(name, depth, tracer):
    want, var, valid, q = closed_form(name, depth)
    assert valid.mean() >= 0.6
    with renderer(name, tracer) as rec:
        img = rec.r.render(params(depth, CONVERGENCE_SPP, seed=9))[..., :3]
        assert rec.r.trace_path() == tracer
    z = ps.z_scores(img, want, var, 1.0 / CONVERGENCE_SPP, q=q)[valid]
    print(f"{name} depth {depth} {tracer}: q = {q:.3g}, largest z {z.max():.2f} over {z.size} cells")
    assert z.max() <= Z_ACCEPT, (name, depth, tracer, float(z.max()))


# ---- c. csg32 and its kernel forms -----------------------------------------------------------------
CSG32_BUILDS = ["-DWO_SKY_RAYS=0", "", "-DWO_CAM_SKY_TILES=0"]  # "" is the default, WO_SKY_RAYS=2


def test_csg32_small_blocks_match_the_reference(monkeypatch):
    frames = {}
    keys = set()
    for tracer in ("jit", "interpreter"):
        for flags in CSG32_BUILDS:  # the interpreter is built ahead of time: the flags must not reach it
            monkeypatch.setenv("WOLOLO_JIT_FLAGS", flags)
            with renderer("csg32_small", tracer) as rec:
                frames[tracer, flags] = rec.r.render(params(8, CSG32_SPP, seed=9))
                assert rec.r.trace_path() == tracer
                if tracer == "jit":
                    keys.add(rec.r.kernel_info()["key"])
    assert len(keys) == len(CSG32_BUILDS), keys  # the switches took effect: three kernels
    first = frames["jit", CSG32_BUILDS[0]]
    for k, f in frames.items():
        assert f.tobytes() == first.tobytes(), k
    mean, var, n = reference("csg32_small", 8)
    bm, bv = ps.block_cells(mean, var)
    z = ps.z_scores(ps.block_cells(first[..., :3].astype(np.float64), var)[0], bm, bv, 1.0 / CSG32_SPP + 1.0 / n)
    print(f"csg32_small: largest block z {z.max():.2f} over {z.size} cells")
    assert z.max() <= Z_ACCEPT, float(z.max())
