"""GPU: mass properties by ray-grid integration (wo_renderer_mass_sums_device,
wo_renderer_mass_properties).  Every field of Wo_MassSums equals the integers of the CPU
reference (tests/mass_support.py: the span reference's crossings of the grid's rays, summed in
Python integers), or closed-form integers where every ray is one whole span."""
import ctypes

import numpy as np
import pytest

import mass_support as ms
import span_support as sp
import test_gpu_rays as tgr
import test_mass as tm
from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl

pytestmark = pytest.mark.gpu

SCENES = ["csg32", "csg32_nested", "csg256_chain", "rtiow_cover"]
FIELDS = ("lo", "hi", "rays", "rays_hit", "crossings")
# the kernel's other forms (query_launch.hip mass_tile / mass_window / mass_reduce / mass_block_flush): the
# same integers
FORMS = [{"WOLOLO_MASS_TILE": "64x1"}, {"WOLOLO_MASS_FLUSH": "wave"}, {"WOLOLO_MASS_WINDOW": "8"},
         {"WOLOLO_MASS_REDUCE": "shfl"},
         {"WOLOLO_MASS_REDUCE": "lds", "WOLOLO_MASS_TILE": "64x1", "WOLOLO_MASS_WINDOW": "8"}]


@pytest.fixture(scope="module")
def span_lib(tmp_path_factory):
    return sp.build_span_ref(tmp_path_factory.mktemp("span_ref"))


def _buffer(fill=0):
    import torch
    return torch.full((24,), fill, dtype=torch.int64, device="cuda")  # a Wo_MassSums


def _read(buf):
    import torch
    torch.cuda.synchronize()
    w = [int(x) for x in buf.cpu().numpy().view(np.uint64)]
    assert w[23] == 0, "Wo_MassSums.reserved was written"
    return {"lo": w[0:10], "hi": w[10:20], "sums": [a + (b << 32) for a, b in zip(w[0:10], w[10:20])], "rays": w[20],
            "rays_hit": w[21], "crossings": w[22]}


def _device(r, g, buf=None):
    """The device form on the current stream into a zeroed (or the given) buffer."""
    import torch
    buf = _buffer() if buf is None else buf
    r.mass_sums_device(g, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return _read(buf)


def _same(got, exp, what):
    bad = {k: (got[k], exp[k]) for k in FIELDS if got[k] != exp[k]}
    assert not bad, f"{what}: not the reference's integers: {bad}"


def _zero(rays):
    return {"lo": [0] * 10, "hi": [0] * 10, "sums": [0] * 10, "rays": rays, "rays_hit": 0, "crossings": 0}


@pytest.mark.parametrize("scene", SCENES)
def test_sums_equal_the_reference(span_lib, scene, monkeypatch):
    """67 x 45 cells (partial waves, partial tiles and strips) of the scene's box along each axis:
    the device form, two workgroups (each lane accumulates over many trips), the host form, and
    the kernel's other forms."""
    r = tgr._renderer(scene)
    sc = sp.SpanScene(span_lib, r)
    for axis in range(3):
        g = ms.grid_of(*sp.BOXES[scene], axis, 67, 45)
        exp = ms.reference_sums(sc, g)
        assert exp["rays"] == 67 * 45 and 0 < exp["rays_hit"] and exp["crossings"] >= 2 * exp["rays_hit"] - exp["rays"]
        _same(_device(r, g), exp, f"{scene} axis {axis}")
        assert r.ray_path() == "interpreter"
        props, sums = r.mass_properties(g)
        _same(sums.as_dict(), exp, f"{scene} axis {axis} host form")
        ms.assert_props_close(ms.props_dict(props), ms.finalise(g, exp), 1e-12, (scene, axis))
        for form in [{}] + (FORMS if axis == 0 else FORMS[-1:]):
            for k, v in form.items():
                monkeypatch.setenv(k, v)
            if form:
                _same(_device(r, g), exp, f"{scene} axis {axis} {form}")
            monkeypatch.setenv("WOLOLO_RAY_BLOCKS", "2")
            _same(_device(r, g), exp, f"{scene} axis {axis} two workgroups {form}")
            for k in list(form) + ["WOLOLO_RAY_BLOCKS"]:
                monkeypatch.delenv(k)
    r.close()


@pytest.mark.parametrize("nu,nv", [(1, 1), (1, 130), (130, 1)])
def test_edge_grids(span_lib, nu, nv, monkeypatch):
    r = tgr._renderer("csg32")
    sc = sp.SpanScene(span_lib, r)
    for axis in range(3):
        g = ms.grid_of(*sp.BOXES["csg32"], axis, nu, nv)
        exp = ms.reference_sums(sc, g)
        assert exp["rays"] == nu * nv
        _same(_device(r, g), exp, f"{nu} x {nv} axis {axis}")
        monkeypatch.setenv("WOLOLO_RAY_BLOCKS", "2")
        _same(_device(r, g), exp, f"{nu} x {nv} axis {axis} two workgroups")
        monkeypatch.setenv("WOLOLO_MASS_TILE", "64x1")
        _same(_device(r, g), exp, f"{nu} x {nv} axis {axis} strips")
        monkeypatch.delenv("WOLOLO_MASS_TILE")
        monkeypatch.delenv("WOLOLO_RAY_BLOCKS")
    r.close()


def test_clip_boxes(span_lib):
    """A box strictly inside csg32's floor slab (y in [-0.5, 0], away from the crater): every ray
    starts inside and ends inside, so the solid is the box; and a box wholly outside the scene."""
    r = tgr._renderer("csg32")
    sc = sp.SpanScene(span_lib, r)
    for axis in range(3):
        g = ms.grid_of((-5.0, -0.4, -5.0), (-1.0, -0.1, -1.0), axis, 67, 45)
        p = wl.mass_grid_plan(g)
        exp = ms.reference_sums(sc, g)
        assert exp["crossings"] == 0 and exp["rays_hit"] == exp["rays"] and exp["sums"][0] == 67 * 45 * (p.q1 - p.q0)
        _same(_device(r, g), exp, f"inside the slab, axis {axis}")
        props, _ = r.mass_properties(g)
        # -0.4 and -0.1 are not dyadic: the faces round in fp32 (2^-24 relative each) and, along y, the
        # extent of 0.3 is quantised in steps of 2^-21 (k = 21): 2^-21 / 0.3 = 1.6e-6 at the most
        assert abs(props.volume - 4.0 * 0.3 * 4.0) <= 2e-6 * 4.8
        g = ms.grid_of((-5.0, 50.0, -5.0), (5.0, 51.0, 5.0), axis, 67, 45)
        exp = ms.reference_sums(sc, g)
        assert exp == _zero(67 * 45)
        _same(_device(r, g), exp, f"outside the scene, axis {axis}")
        props, _ = r.mass_properties(g)
        assert props.volume == 0.0 and tuple(props.centroid) == (0.0, 50.5, 0.0) and not any(props.inertia)
        assert props.rays == 67 * 45 and props.projected_area == 0.0
    r.close()


def test_empty_scene():
    r = wl.Renderer("empty", max_nodes=4)
    for axis in range(3):
        g = ms.grid_of((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), axis, 67, 45)
        _same(_device(r, g), _zero(67 * 45), f"empty scene, axis {axis}")
        props, sums = r.mass_properties(g)
        _same(sums.as_dict(), _zero(67 * 45), "empty scene, host form")
        assert props.volume == 0.0 and props.rays == 67 * 45
    r.close()


def _whole_span_sums(g):
    """Closed-form Wo_MassSums when every ray of the row range is the span [q0, q1]: the ten totals
    from sum i' = nu^2 and sum i'^2 = nu (4 nu^2 - 1) / 3 (likewise over the rows), and the limbs
    from the per-ray terms in uint64."""
    p = wl.mass_grid_plan(g)
    q0, q1, nu = p.q0, p.q1, g.nu
    m0, m1, m2 = q1 - q0, q1 ** 2 - q0 ** 2, q1 ** 3 - q0 ** 3
    rows = lambda n: (n * n, n * (4 * n * n - 1) // 3)  # sum and sum of squares of the first n odd numbers
    si, sii = rows(nu)
    sj = rows(g.v_begin + g.v_count)[0] - rows(g.v_begin)[0]
    sjj = rows(g.v_begin + g.v_count)[1] - rows(g.v_begin)[1]
    nr = nu * g.v_count
    totals = [m0 * nr, m0 * si * g.v_count, m0 * sj * nu, m1 * nr, m0 * sii * g.v_count, m0 * sjj * nu, m2 * nr,
              m0 * si * sj, m1 * si * g.v_count, m1 * sj * nu]
    U = np.uint64
    i2 = (2 * np.arange(nu, dtype=U) + U(1))[None, :]
    j2 = (2 * np.arange(g.v_begin, g.v_begin + g.v_count, dtype=U) + U(1))[:, None]
    one = np.ones((g.v_count, nu), dtype=U)
    a0, a1, a2 = U(m0), U(m1), U(m2)
    terms = [a0 * one, a0 * i2 * one, a0 * j2 * one, a1 * one, a0 * i2 * i2 * one, a0 * j2 * j2 * one, a2 * one,
             a0 * i2 * j2, a1 * i2 * one, a1 * j2 * one]
    lo = [int((t & U(0xFFFFFFFF)).sum(dtype=U)) for t in terms]
    hi = [int((t >> U(32)).sum(dtype=U)) for t in terms]
    assert [a + (b << 32) for a, b in zip(lo, hi)] == totals
    return {"lo": lo, "hi": hi, "sums": totals, "rays": nr, "rays_hit": nr, "crossings": 0}


def test_exact_integer_cases():
    """A lone half-space y <= 0 fills a box below it: every ray is [q0, q1].  64 x 64, and the last
    64 rows of the 32768 x 32768 grid: the largest i', j' and m2 and the high limbs."""
    r = wl.Renderer("halfspace", max_nodes=4)
    r.halfspace((0.0, 1.0, 0.0))
    box = ((-1.0, -2.0, -1.0), (1.0, -0.5, 1.0))
    for axis in range(3):
        g = ms.grid_of(*box, axis, 64, 64)
        _same(_device(r, g), _whole_span_sums(g), f"64 x 64 axis {axis}")
    g = ms.grid_of(*box, 1, 32768, 32768, 32768 - 64, 64)
    exp = _whole_span_sums(g)
    assert max(exp["hi"]) > 1 << 32 and exp["sums"][6] > 1 << 64
    _same(_device(r, g), exp, "the last 64 rows of 32768 x 32768")
    r.close()


def test_parts_add_up_and_calls_accumulate(span_lib):
    scene = "csg32_nested"
    r = tgr._renderer(scene)
    box = sp.BOXES[scene]
    whole = ms.grid_of(*box, 0, 67, 45)
    exp = ms.reference_sums(sp.SpanScene(span_lib, r), whole)
    buf = _buffer()
    got = None
    for v_begin, v_count in ((0, 7), (7, 30), (37, 8)):
        got = _device(r, ms.grid_of(*box, 0, 67, 45, v_begin, v_count), buf)
    _same(got, exp, "three row ranges into one buffer")
    twice = {k: [2 * x for x in exp[k]] if isinstance(exp[k], list) else 2 * exp[k] for k in exp}
    _same(_device(r, whole, buf), twice, "a second call without zeroing")
    first = _device(r, whole)
    for _ in range(4):
        assert _device(r, whole) == first
    _same(first, exp, "repeated")
    r.close()


def _hip_runtime():
    """The HIP runtime this process has loaded (the one torch's streams belong to)."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, paths
    hip = ctypes.CDLL(paths[0])
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    return hip


def test_ordering(span_lib):
    """Behind a hipMemsetAsync on a stream that is not the default one; the host form against the
    device form; and a scene edit between two calls."""
    import torch
    r = wl.Renderer("edit", max_nodes=4096)
    scenes.build("csg32", r)
    r.set_tracer("interpreter")
    g = ms.grid_of(*sp.BOXES["csg32"], 1, 67, 45)
    exp0 = ms.reference_sums(sp.SpanScene(span_lib, r), g)
    buf = _buffer(fill=0x5555555555555555)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert _hip_runtime().hipMemsetAsync(buf.data_ptr(), 0, 192, side.cuda_stream) == 0
    r.mass_sums_device(g, buf.data_ptr(), side.cuda_stream)
    side.synchronize()
    _same(_read(buf), exp0, "behind a hipMemsetAsync on a side stream")
    props, sums = r.mass_properties(g)
    _same(sums.as_dict(), exp0, "host form")
    # the top of the scene's box is empty: a sphere put there is new volume
    ball = r.sphere(0.5)
    r.union(wl.arg(ball, (0.0, 2.45, 5.5)), wl.arg(ball, (0.2, 2.45, 5.5)))
    exp1 = ms.reference_sums(sp.SpanScene(span_lib, r), g)
    assert exp1["sums"][0] > exp0["sums"][0] and exp1["rays_hit"] >= exp0["rays_hit"]
    _same(_device(r, g), exp1, "after the edit")
    r.close()


def test_sphere_end_to_end(span_lib):
    r = wl.Renderer("sphere", max_nodes=16)
    ms.build_sphere(r)
    g = ms.grid_of(*ms.SOLID_BOX, 2, 251, 251)
    props, sums = r.mass_properties(g)
    got = ms.props_dict(props)
    err = ms.errors(got, ms.exact_sphere())
    print("sphere 251 x 251, axis 2:", err)
    assert all(e <= t for e, t in zip(err, tm.TOLERANCE["sphere", 251])), err
    exp = ms.reference_sums(sp.SpanScene(span_lib, r), g)
    _same(sums.as_dict(), exp, "sphere 251 x 251")
    ms.assert_props_close(got, ms.finalise(g, exp), 1e-12, "sphere 251 x 251")
    assert props.rays == 251 * 251 and props.crossings == exp["crossings"]
    r.close()
