"""Mass properties by ray-grid integration, the host side (CPU only): the ABI of the four structs,
wo_mass_grid_plan against its float32 numpy restatement, the bad grids, the loud failure without
a device, csrc/mass.c's stand-alone driver under ASan + UBSan, wo_mass_properties_from_sums
against the float64 restatement, and the reference the GPU tests compare against
(tests/mass_support.py) judged against solids with closed forms."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import mass_support as ms
import span_support as sp
from csgrenderer_amd import wololo as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csgrenderer_amd", "csrc")


@pytest.fixture(scope="module")
def span_lib(tmp_path_factory):
    return sp.build_span_ref(tmp_path_factory.mktemp("span_ref"))


@pytest.mark.parametrize("cname,mirror,size", [("Wo_MassGrid", wl.MassGrid, 48), ("Wo_MassPlan", wl.MassPlan, 44),
                                               ("Wo_MassSums", wl.MassSums, 192),
                                               ("Wo_MassProperties", wl.MassProperties, 152)])
def test_mass_abi_layout(cname, mirror, size):
    assert ctypes.sizeof(mirror) == size == wl.abi_layout(cname)
    for fname, _ in mirror._fields_:
        assert wl.abi_layout(cname, fname) == getattr(mirror, fname).offset, (cname, fname)
    assert wl.MASS_MAX_CELLS == 32768


def _plan_matches(lo, hi, axis, nu, nv):
    got = wl.mass_grid_plan(ms.grid_of(lo, hi, axis, nu, nv))
    want = ms.np_plan(lo, hi, axis, nu, nv)
    for name in ("o_axis", "pad", "t_max", "scale", "u0", "hu", "v0", "hv"):
        assert np.float32(getattr(got, name)).tobytes() == np.float32(want[name]).tobytes(), (name, lo, hi, axis)
    assert (got.k, got.q0, got.q1) == (want["k"], want["q0"], want["q1"]), (lo, hi, axis)
    assert got.q1 <= 1 << 20 and got.q0 <= got.q1
    return got


def test_plan_matches_the_numpy_restatement():
    rng = np.random.default_rng(5)
    for _ in range(300):
        centre = rng.normal(size=3) * 10.0 ** rng.integers(-3, 4)
        half = 10.0 ** rng.uniform(-4, 4, size=3)
        lo, hi = (centre - half).astype(np.float32), (centre + half).astype(np.float32)
        if not (lo < hi).all():
            continue
        _plan_matches(lo, hi, int(rng.integers(0, 3)), int(rng.integers(1, 32769)), int(rng.integers(1, 32769)))
    for axis in range(3):
        # huge and tiny extents (k negative and large), an extent below pad's last bit, the largest counts
        huge = _plan_matches((-1e30, -2e29, -3e28), (1e30, 2e29, 3e28), axis, 7, 32768)
        assert huge.k < 0 and huge.q0 == 0
        tiny = _plan_matches((1.0, 1.0, 1.0), np.nextafter(np.float32(1.0), np.float32(2.0)).repeat(3), axis, 32768, 1)
        assert tiny.k == 28 and tiny.q0 == 1 << 19 and tiny.q1 == (1 << 19) + 32
        small = _plan_matches((-1e-30, -1e-30, -1e-30), (1e-30, 1e-30, 1e-30), axis, 3, 5)
        assert small.k == 28 and small.q0 == small.q1 == 1 << 19
        unit = _plan_matches((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), axis, 1, 1)
        assert (unit.k, unit.q0, unit.q1) == (19, 1 << 10, (1 << 19) + (1 << 10))
        _plan_matches((-8.0, -8.0, -8.0), (8.0 - 2.0 ** -9, 8.0, 8.0), axis, 255, 257)


BAD_GRIDS = {
    "nan": dict(lo=(np.nan, -1, -1)), "inf": dict(hi=(1, np.inf, 1)), "minus inf": dict(lo=(-1, -1, -np.inf)),
    "lo == hi": dict(lo=(-1, 1, -1)), "lo > hi": dict(hi=(1, 1, -2)), "axis 3": dict(axis=3), "nu 0": dict(nu=0),
    "nv 0": dict(nv=0, v_count=1), "nu 32769": dict(nu=32769), "nv 32769": dict(nv=32769), "v_count 0": dict(v_count=0),
    "v_begin = nv": dict(v_begin=4, v_count=1), "rows past nv": dict(v_begin=2, v_count=3),
    "rows wrap": dict(v_begin=1, v_count=0xFFFFFFFF), "reserved": dict(reserved=1),
    "extent overflows": dict(lo=(-3e38, -1, -1), hi=(3e38, 1, 1)),
    "k below -100": dict(lo=(-1e37, -1, -1), hi=(1e37, 1, 1)),
}


def _bad_grid(case):
    kw = dict(lo=(-1, -1, -1), hi=(1, 1, 1), axis=0, nu=4, nv=4, v_begin=0, v_count=4, reserved=0)
    kw.update(BAD_GRIDS[case])
    g = ms.grid_of(kw["lo"], kw["hi"], kw["axis"], kw["nu"], kw["nv"], kw["v_begin"], kw["v_count"])
    g.reserved = kw["reserved"]
    return g


@pytest.mark.parametrize("case", sorted(BAD_GRIDS))
def test_bad_grid_is_refused(case):
    g = _bad_grid(case)
    lib = wl.load()
    wl.clear_error()
    assert lib.wo_mass_grid_plan(ctypes.byref(g), ctypes.byref(wl.MassPlan())) == -1
    assert "mass grid" in wl.last_error()
    wl.clear_error()
    assert lib.wo_mass_properties_from_sums(ctypes.byref(g), ctypes.byref(wl.MassSums()),
                                            ctypes.byref(wl.MassProperties())) == -1
    assert "mass grid" in wl.last_error()
    with pytest.raises(wl.WololoError, match="mass grid"):
        wl.mass_grid_plan(g)


def test_mass_without_device_fails_loudly(hostonly):
    r = wl.Renderer("nodev", max_nodes=4)
    r.sphere(1.0)
    g = ms.grid_of((-1, -1, -1), (1, 1, 1), 0, 4, 4)
    for call in (lambda: r.mass_sums_device(g, 0x1000), lambda: r.mass_properties(g)):
        wl.clear_error()
        with pytest.raises(wl.WololoError, match="device"):
            call()
    assert r.lib.wo_renderer_mass_sums_device(r.ptr, ctypes.byref(g), 0x1000, None) == -1
    assert r.lib.wo_renderer_mass_properties(r.ptr, ctypes.byref(g), ctypes.byref(wl.MassProperties()), None) == -1
    assert r.ray_path() == "none"
    r.close()


def test_mass_driver_runs_clean_under_sanitizers():
    """csrc/mass.c with tests/host/mass_main.c (its own main), built with ASan + UBSan."""
    run = subprocess.run(["make", "-C", CSRC, "mass-asan"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mass driver: ok" in run.stdout and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr


# ---- the reference against closed forms ----
_REF = {}


def _reference(span_lib, name, build, g_args):
    """Reference sums of a small scene on a grid, made once and shared."""
    key = (name, g_args)
    if key not in _REF:
        r = wl.Renderer(name, max_nodes=32)
        build(r)
        g = ms.grid_of(*g_args)
        _REF[key] = (g, ms.reference_sums(sp.SpanScene(span_lib, r), g))
        r.close()
    return _REF[key]


DYADIC = ((-1.0, -0.5, -1.5), (0.5, 1.5, 1.0))  # the solid box: faces on multiples of 0.5
DYADIC_CLIP = ((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0))  # 16 x 8 cells of 0.25 x 0.5


def build_dyadic_box(r):
    lo, hi = DYADIC
    halves = []
    for a in range(3):
        for sign, face in ((1.0, hi[a]), (-1.0, lo[a])):  # sign (x[a] - face) <= 0
            n, off = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
            n[a], off[a] = sign, face
            halves.append(wl.arg(r.halfspace(tuple(n)), tuple(off)))
    node = r.intersection(halves[0], halves[1])
    for half in halves[2:]:
        node = r.intersection(wl.arg(node), half)


def _box_exact(lo, hi):
    lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    e = hi - lo
    V = float(e.prod())
    return {"volume": V, "centroid": 0.5 * (lo + hi),
            "inertia": np.diag([V / 12.0 * (e[1] ** 2 + e[2] ** 2), V / 12.0 * (e[0] ** 2 + e[2] ** 2),
                                V / 12.0 * (e[0] ** 2 + e[1] ** 2)])}


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_dyadic_box_is_exact(hostonly, span_lib, axis):
    """pad is a power of two, so the faces' parameters are exact, and the faces lie on cell
    boundaries: the column model is the box itself."""
    g, d = _reference(span_lib, "dyadic", build_dyadic_box, (*DYADIC_CLIP, axis, 16, 8))
    exact = _box_exact(*DYADIC)
    for got in (ms.finalise(g, d), ms.props_dict(wl.mass_properties_from_sums(g, ms.to_struct(d)))):
        err = ms.errors(got, exact)
        print("dyadic box, axis", axis, err)
        assert max(err) <= 1e-9, err
    u, v = (axis + 1) % 3, (axis + 2) % 3
    e = np.array(DYADIC[1]) - np.array(DYADIC[0])
    assert d["rays"] == 128 and d["rays_hit"] == round(e[u] / 0.25) * round(e[v] / 0.5) and d["crossings"] == 2 * d["rays_hit"]


# 4 x the error of the float64 restatement on the reference's sums, worst of the three axes, measured on
# the CPU (the measured value beside each): (volume relative, centroid absolute, inertia relative to its
# largest entry) at 61 x 61 and 251 x 251 cells of SOLID_BOX
TOLERANCE = {
    ("sphere", 61): (3.7e-4, 2.2e-3, 3.6e-3),   # measured 9.189e-05, 5.447e-04, 8.956e-04
    ("sphere", 251): (1.2e-4, 1.9e-5, 1.5e-4),  # measured 2.922e-05, 4.624e-06, 3.543e-05
    ("shell", 61): (1.6e-3, 3.5e-3, 4.3e-3),    # measured 3.994e-04, 8.693e-04, 1.065e-03
    ("shell", 251): (1.4e-4, 4.4e-5, 1.7e-4),   # measured 3.383e-05, 1.076e-05, 4.157e-05
    ("lens", 61): (2.5e-3, 2.3e-3, 8.9e-3),     # measured 6.174e-04, 5.729e-04, 2.224e-03
    ("lens", 251): (2.5e-5, 1.7e-4, 3.5e-4),    # measured 6.216e-06, 4.246e-05, 8.690e-05
}


@pytest.mark.parametrize("solid", sorted(ms.SOLIDS))
def test_closed_forms(hostonly, span_lib, solid):
    build, exact = ms.SOLIDS[solid]
    exact = exact()
    worst = {}
    for n in (61, 251):
        worst[n] = np.zeros(3)
        for axis in range(3):
            g, d = _reference(span_lib, solid, build, (*ms.SOLID_BOX, axis, n, n))
            got = ms.finalise(g, d)
            err = ms.errors(got, exact)
            print(solid, n, "axis", axis, "volume, centroid, inertia errors", err)
            assert all(e <= t for e, t in zip(err, TOLERANCE[solid, n])), (solid, n, axis, err)
            worst[n] = np.maximum(worst[n], err)
            # and csrc/mass.c's finalisation of the same sums
            ms.assert_props_close(ms.props_dict(wl.mass_properties_from_sums(g, ms.to_struct(d))), got, 1e-12,
                                  (solid, n, axis))
    # the silhouette's error oscillates with the cell count, but between these two counts the worst
    # axis improves at least threefold in every quantity on the reference (measured above)
    assert (worst[251] < worst[61]).all(), (solid, worst)


HEMI_N = 251
# the sphere of ms.build_sphere cut in half by a face of the clip box: which face, as (side, axis role)
HEMI_CASES = ["near", "far", "side"]
# 4 x measured, as TOLERANCE: (volume relative, centroid absolute, worst axis); measured values beside
HEMI_TOLERANCE = {"near": (1.2e-4, 5.0e-5),  # measured 2.921e-05, 1.245e-05
                  "far": (1.2e-4, 5.0e-5),   # measured 2.921e-05, 1.245e-05
                  "side": (6.5e-5, 8.6e-5)}  # measured 1.617e-05, 2.154e-05


def _hemi_grid(case, axis):
    lo, hi = [list(x) for x in ms.SOLID_BOX]
    cut = axis if case != "side" else (axis + 1) % 3
    (hi if case == "far" else lo)[cut] = ms.CENTRE[cut]
    return (tuple(lo), tuple(hi), axis, HEMI_N, HEMI_N), cut, (-1.0 if case == "far" else 1.0)


@pytest.mark.parametrize("case", HEMI_CASES)
def test_clip_box_cuts_the_sphere_in_half(hostonly, span_lib, case):
    """The box is a true clip box: a near face inside the solid (rays start inside, spans clamp to
    q0), a far face inside it (rays end inside and close at q1), and a side face."""
    R = ms.R_OUT
    V = 2.0 / 3.0 * math.pi * R ** 3
    for axis in range(3):
        g_args, cut, sign = _hemi_grid(case, axis)
        g, d = _reference(span_lib, "sphere", ms.build_sphere, g_args)
        got = ms.finalise(g, d)
        want_c = np.array(ms.CENTRE)
        want_c[cut] += sign * 3.0 * R / 8.0
        err = (abs(got["volume"] - V) / V, float(np.abs(got["centroid"] - want_c).max()))
        print("hemisphere", case, "axis", axis, err)
        assert all(e <= t for e, t in zip(err, HEMI_TOLERANCE[case])), (case, axis, err)
        ms.assert_props_close(ms.props_dict(wl.mass_properties_from_sums(g, ms.to_struct(d))), got, 1e-12, (case, axis))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_half_space_fills_the_box(hostonly, span_lib, axis):
    """y <= 0 and a box below it: no ray has an event along x or z, along y none either (they start
    and end inside); every span is [q0, q1] and the volume is the box's."""
    box = ((-1.0, -2.0, -1.0), (1.0, -0.5, 1.0))
    g, d = _reference(span_lib, "halfspace", lambda r: r.halfspace((0.0, 1.0, 0.0)), (*box, axis, 64, 64))
    p = ms.np_plan(*box, axis, 64, 64)
    assert d["crossings"] == 0 and d["rays"] == d["rays_hit"] == 4096 and d["sums"][0] == 4096 * (p["q1"] - p["q0"])
    got = ms.props_dict(wl.mass_properties_from_sums(g, ms.to_struct(d)))
    exact = _box_exact(*box)
    assert max(ms.errors(got, exact)) <= 1e-12
    ms.assert_props_close(got, ms.finalise(g, d), 1e-12, axis)
