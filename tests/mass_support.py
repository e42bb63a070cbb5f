"""Shared by tests/test_mass.py and tests/test_gpu_mass.py (test helper, no fixture): the CPU
reference of the mass-properties query.  The grid's rays are built in float32 numpy exactly as
renderer_ext.h states them, tests/span_support.py's reference (tests/host/span_ref.c over the
oracle's functions) lists every crossing of each, Python integers form the ten sums and the
counters, and a float64 restatement of the finalisation, written from the header's formulas,
gives the properties.  Also the closed-form solids the CPU and GPU tests share."""
import math

import numpy as np
from numpy.polynomial import Polynomial as Poly

import span_support as sp
from csgrenderer_amd import wololo as wl

F32 = np.float32
PAD = F32(2.0 ** -9)
MAX_REF = 64  # the reference's crossing cap: every ray of every grid used here must stay within it


def np_plan(lo, hi, axis, nu, nv):
    """Wo_MassPlan in float32 numpy, one rounding per operation: a dict of its fields."""
    lo, hi = np.asarray(lo, dtype=F32), np.asarray(hi, dtype=F32)
    u, v = (axis + 1) % 3, (axis + 2) % 3
    o_axis = F32(lo[axis] - PAD)
    t_max = F32(PAD + F32(hi[axis] - lo[axis]))
    _, e = np.frexp(t_max)
    k = 20 - int(e)
    scale = F32(2.0 ** k)
    q = lambda t: int(np.rint(F32(F32(t) * scale)))
    return {"o_axis": o_axis, "pad": PAD, "t_max": t_max, "scale": scale, "k": k, "q0": q(PAD), "q1": q(t_max),
            "u0": lo[u], "hu": F32(F32(hi[u] - lo[u]) / F32(2 * nu)), "v0": lo[v],
            "hv": F32(F32(hi[v] - lo[v]) / F32(2 * nv))}


def grid_of(lo, hi, axis, nu, nv, v_begin=0, v_count=None):
    return wl.mass_grid(lo, hi, axis, nu, nv, v_begin, v_count)


def grid_rays(g):
    """The Wo_Ray rows of the grid's row range, row-major (j, then i), and their i' and j'."""
    axis, nu = g.axis, g.nu
    p = np_plan(list(g.lo), list(g.hi), axis, nu, g.nv)
    u, v = (axis + 1) % 3, (axis + 2) % 3
    i2 = (2 * np.arange(nu, dtype=np.int64) + 1)
    j2 = (2 * np.arange(g.v_begin, g.v_begin + g.v_count, dtype=np.int64) + 1)
    cu = p["u0"] + i2.astype(F32) * p["hu"]  # float32: the product rounds, then the sum
    cv = p["v0"] + j2.astype(F32) * p["hv"]
    assert cu.dtype == F32 and cv.dtype == F32
    o = np.zeros((len(j2), nu, 3), dtype=F32)
    o[:, :, axis] = p["o_axis"]
    o[:, :, u] = cu[None, :]
    o[:, :, v] = cv[:, None]
    d = np.zeros((len(j2) * nu, 3), dtype=F32)
    d[:, axis] = 1.0
    rays = sp.ray_rows(o.reshape(-1, 3), d, p["t_max"])
    return rays, np.tile(i2, len(j2)), np.repeat(j2, nu), p


def sums_of_crossings(ref, i2, j2, p):
    """The Wo_MassSums of rays whose crossings the span reference lists: a dict like
    wl.MassSums.as_dict().  Per ray in uint64 (every term is below 2^63), then Python integers."""
    count = ref["count"].astype(np.int64)
    assert count.max(initial=0) <= MAX_REF, f"a ray has {count.max()} crossings: pick another grid"
    n = len(count)
    U = np.uint64
    q0, q1 = U(p["q0"]), U(p["q1"])
    qa = np.full(n, q0, dtype=U)
    m0, m1, m2 = (np.zeros(n, dtype=U) for _ in range(3))

    def close(sel, qb):
        a, b = qa[sel], qb
        m0[sel] += b - a
        m1[sel] += b * b - a * a
        m2[sel] += b * b * b - a * a * a

    for k in range(int(count.max(initial=0))):
        on = count > k
        prod = ref["t"][:, k] * p["scale"]
        assert prod.dtype == F32
        c = np.clip(np.rint(prod).astype(np.int64), int(q0), int(q1)).astype(U)
        enters = on & (ref["after"][:, k] != 0)
        leaves = on & (ref["after"][:, k] == 0)
        close(leaves, c[leaves])
        qa[enters] = c[enters]
    still = ((ref["inside0"].astype(np.int64) + count) % 2) == 1
    close(still, np.full(int(still.sum()), q1, dtype=U))
    i2, j2 = i2.astype(U), j2.astype(U)
    terms = [m0, m0 * i2, m0 * j2, m1, m0 * i2 * i2, m0 * j2 * j2, m2, m0 * i2 * j2, m1 * i2, m1 * j2]
    lo = [sum((t & U(0xFFFFFFFF)).tolist()) for t in terms]
    hi = [sum((t >> U(32)).tolist()) for t in terms]
    return {"sums": [a + (b << 32) for a, b in zip(lo, hi)], "lo": lo, "hi": hi, "rays": n,
            "rays_hit": int((m0 > 0).sum()), "crossings": int(count.sum())}


def reference_sums(span_scene, g):
    """The reference's Wo_MassSums of the grid's row range on a span_support.SpanScene."""
    rays, i2, j2, p = grid_rays(g)
    return sums_of_crossings(span_scene.reference(rays, MAX_REF), i2, j2, p)


def add_sums(a, b):
    out = {k: [x + y for x, y in zip(a[k], b[k])] for k in ("sums", "lo", "hi")}
    out.update({k: a[k] + b[k] for k in ("rays", "rays_hit", "crossings")})
    return out


def to_struct(d):
    s = wl.MassSums()
    s.lo[:] = d["lo"]
    s.hi[:] = d["hi"]
    s.rays, s.rays_hit, s.crossings = d["rays"], d["rays_hit"], d["crossings"]
    return s


def finalise(g, d):
    """renderer_ext.h's finalisation restated in float64: dict of volume, centroid[3], inertia[3,3],
    projected_area, cell[3]."""
    axis = g.axis
    u, v = (axis + 1) % 3, (axis + 2) % 3
    p = np_plan(list(g.lo), list(g.hi), axis, g.nu, g.nv)
    S = [float(x) for x in d["sums"]]  # a Python integer to the nearest double
    h, hu, hv = 2.0 ** -p["k"], float(p["hu"]), float(p["hv"])
    A = (2.0 * hu) * (2.0 * hv)
    out = {"projected_area": d["rays_hit"] * A, "cell": np.array([2.0 * hu, 2.0 * hv, h])}
    if d["sums"][0] == 0:
        out.update(volume=0.0, centroid=0.5 * (np.array(list(g.lo), dtype=np.float64) + np.array(list(g.hi))),
                   inertia=np.zeros((3, 3)))
        return out
    V = A * h * S[0]
    mean = np.array([hu * S[1] / S[0], hv * S[2] / S[0], 0.5 * h * S[3] / S[0]])
    E = np.zeros((3, 3))
    E[0, 0] = A * h * (hu * hu * S[4] + hu * hu / 3.0 * S[0])
    E[1, 1] = A * h * (hv * hv * S[5] + hv * hv / 3.0 * S[0])
    E[2, 2] = A * h ** 3 / 3.0 * S[6]
    E[0, 1] = E[1, 0] = A * h * hu * hv * S[7]
    E[0, 2] = E[2, 0] = A * h * h / 2.0 * hu * S[8]
    E[1, 2] = E[2, 1] = A * h * h / 2.0 * hv * S[9]
    C = E - V * np.outer(mean, mean)
    local = np.trace(C) * np.eye(3) - C
    world = [u, v, axis]
    inertia = np.zeros((3, 3))
    centroid = np.zeros(3)
    origin = [float(g.lo[u]), float(g.lo[v]), float(p["o_axis"])]
    for a in range(3):
        centroid[world[a]] = origin[a] + mean[a]
        for b in range(3):
            inertia[world[a], world[b]] = local[a, b]
    out.update(volume=V, centroid=centroid, inertia=inertia)
    return out


def props_dict(m):
    """A wl.MassProperties as finalise() returns them."""
    return {"volume": m.volume, "centroid": np.array(list(m.centroid)), "inertia": np.array(list(m.inertia)).reshape(3, 3),
            "projected_area": m.projected_area, "cell": np.array(list(m.cell))}


def assert_props_close(got, want, rel, what):
    """Every property within rel of the quantity's own scale (the inertia's largest entry, the
    clip box's size for the centroid is the caller's: here the centroid's own norm + 1)."""
    scale_i = np.abs(want["inertia"]).max() + 1e-300
    assert abs(got["volume"] - want["volume"]) <= rel * abs(want["volume"]) + 1e-300, (what, got["volume"], want["volume"])
    assert np.abs(got["centroid"] - want["centroid"]).max() <= rel * (np.abs(want["centroid"]).max() + 1.0), what
    assert np.abs(got["inertia"] - want["inertia"]).max() <= rel * scale_i, (what, got["inertia"], want["inertia"])
    assert abs(got["projected_area"] - want["projected_area"]) <= rel * (abs(want["projected_area"]) + 1e-300), what
    assert np.abs(got["cell"] - want["cell"]).max() <= rel * want["cell"].max(), what


# ---- solids with closed forms ----
CENTRE = (0.3125, -0.1875, 0.4375)  # dyadic, off every cell centre and boundary of the grids used
R_OUT, R_IN = 1.25, 0.75
LENS_R, LENS_A = 1.25, 0.5  # two spheres of radius LENS_R, centres CENTRE -+ LENS_A along x
SOLID_BOX = ((-1.5, -2.0, -1.375), (2.25, 1.5, 2.125))  # contains all three solids with room to spare


def build_sphere(r):
    c = CENTRE
    r.intersection(wl.arg(r.sphere(R_OUT), c), wl.arg(r.sphere(2.0 * R_OUT), c))


def build_shell(r):
    c = CENTRE
    r.difference(wl.arg(r.sphere(R_OUT), c), wl.arg(r.sphere(R_IN), c))


def build_lens(r):
    c = CENTRE
    s = r.sphere(LENS_R)
    r.intersection(wl.arg(s, (c[0] - LENS_A, c[1], c[2])), wl.arg(s, (c[0] + LENS_A, c[1], c[2])))


def _diag(x, y, z):
    return np.diag([x, y, z]).astype(np.float64)


def exact_sphere():
    V = 4.0 / 3.0 * math.pi * R_OUT ** 3
    i = 0.4 * V * R_OUT ** 2
    return {"volume": V, "centroid": np.array(CENTRE), "inertia": _diag(i, i, i)}


def exact_shell():
    V = 4.0 / 3.0 * math.pi * (R_OUT ** 3 - R_IN ** 3)
    i = 0.4 * 4.0 / 3.0 * math.pi * (R_OUT ** 5 - R_IN ** 5)
    return {"volume": V, "centroid": np.array(CENTRE), "inertia": _diag(i, i, i)}


def exact_lens():
    """Two caps of height R - a, as stacks of discs of radius^2 R^2 - x^2, x from a to R in the
    sphere's own frame; the cap formula pi h^2 (3R - h) / 3 is asserted against the integral."""
    R, a = LENS_R, LENS_A
    r2 = Poly([R * R, 0.0, -1.0])
    x = Poly([-a, 1.0])  # distance from the lens's plane of symmetry
    integral = lambda poly: poly.integ()(R) - poly.integ()(a)
    V = 2.0 * math.pi * integral(r2)
    h = R - a
    assert abs(V - 2.0 * math.pi * h * h * (3.0 * R - h) / 3.0) < 1e-12 * V
    axial = 2.0 * (math.pi / 2.0) * integral(r2 * r2)
    transverse = 2.0 * (math.pi / 4.0 * integral(r2 * r2) + math.pi * integral(r2 * x * x))
    return {"volume": V, "centroid": np.array(CENTRE), "inertia": _diag(axial, transverse, transverse)}


SOLIDS = {"sphere": (build_sphere, exact_sphere), "shell": (build_shell, exact_shell), "lens": (build_lens, exact_lens)}


def errors(got, exact):
    """(volume, centroid, inertia) errors of finalised properties against a closed form: the volume's
    relative, the centroid's absolute (largest component), the inertia's largest entry error
    relative to the closed form's largest entry."""
    return (abs(got["volume"] - exact["volume"]) / exact["volume"],
            float(np.abs(got["centroid"] - exact["centroid"]).max()),
            float(np.abs(got["inertia"] - exact["inertia"]).max() / np.abs(exact["inertia"]).max()))
