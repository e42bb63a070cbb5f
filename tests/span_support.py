"""Shared by tests/test_spans.py and tests/test_gpu_spans.py (test helper, no fixture): the
CPU reference of the span query (tests/host/span_ref.c over the oracle's own functions),
expected Wo_RaySpans / Wo_RayCrossing rows from it, the "through rays" batch, and the float32
restatement of point classification."""
import ctypes
import os
import subprocess

import numpy as np

from csgrenderer_amd import wololo as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPANS_DT = np.dtype(wl.RAY_SPANS_FIELDS)
CROSSING_DT = np.dtype(wl.RAY_CROSSING_FIELDS)
# where origins and targets are drawn: test_gpu_rays.BOXES and the chain's box
BOXES = {
    "csg32": ((-6.5, -1.0, -6.5), (6.5, 3.0, 6.5)),
    "csg32_union": ((-6.5, -1.0, -6.5), (6.5, 3.0, 6.5)),
    "csg32_nested": ((-3.0, -1.2, -3.0), (3.0, 4.4, 3.0)),
    "rtiow_cover": ((-11.0, -0.5, -11.0), (11.0, 2.5, 11.0)),
    "csg256_chain": ((-5.0, -0.5, -5.0), (5.0, 3.0, 5.0)),
}
N_THROUGH = 1024
SENTINEL = 0xA5A5A5A5  # every word of a crossing row the query must not write


def build_span_ref(outdir):
    """Compile tests/host/span_ref.c with the oracle Makefile's flags; the loaded library."""
    so = os.path.join(str(outdir), "span_ref.so")
    subprocess.run(["gcc", "-std=c11", "-O2", "-mfma", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                    "-fno-unsafe-math-optimizations", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "oracle"), "-shared", "-o", so,
                    os.path.join(ROOT, "tests", "host", "span_ref.c"), "-lm"], check=True)
    lib = ctypes.CDLL(so)
    lib.span_ref.restype = ctypes.c_int
    lib.span_ref.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + \
        [ctypes.c_void_p] * 7
    return lib


def unit(v):
    """float32 rows normalised in float32."""
    v = np.asarray(v, dtype=np.float32)
    n = np.sqrt((v * v).sum(axis=1, dtype=np.float32), dtype=np.float32)
    return (v / n[:, None]).astype(np.float32)


def ray_rows(o, d, t_max=np.inf):
    rays = np.zeros((len(o), 8), dtype=np.float32)
    rays[:, 0:3] = o
    rays[:, 3] = t_max
    rays[:, 4:7] = d
    return rays


def through_rays(scene, n=N_THROUGH, seed=7):
    """Rays that cross the whole scene: origin and target uniform in the scene's box, then, along
    x or z, the origin put 1.0 outside one face and the target 1.0 outside the opposite one."""
    rng = np.random.default_rng(seed)
    lo, hi = (np.array(v, dtype=np.float64) for v in BOXES[scene])
    o = rng.uniform(lo, hi, size=(n, 3))
    tg = rng.uniform(lo, hi, size=(n, 3))
    axis = 2 * rng.integers(0, 2, size=n)
    fwd = rng.integers(0, 2, size=n).astype(bool)
    rows = np.arange(n)
    o[rows, axis] = np.where(fwd, lo[axis] - 1.0, hi[axis] + 1.0)
    tg[rows, axis] = np.where(fwd, hi[axis] + 1.0, lo[axis] - 1.0)
    o32, tg32 = o.astype(np.float32), tg.astype(np.float32)
    return ray_rows(o32, unit(tg32 - o32))


def rays_valid(rays):
    o, d, t_max = rays[:, 0:3], rays[:, 4:7], rays[:, 3]
    return np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1) & ~np.isnan(t_max)


class SpanScene:
    """A compiled scene as the reference needs it, and expected rows from the reference."""

    def __init__(self, lib, r):
        self.lib = lib
        self.prog, self.nrec, self.nprims = r.program()
        self.nodes = r.program_nodes()
        self.ordpc = np.zeros(max(self.nprims, 1), dtype=np.int64)
        for pc in range(self.nrec):
            if self.prog[pc].op == wl.WO_OP_PRIM:
                self.ordpc[self.prog[pc].u1] = pc

    def reference(self, rays, max_out):
        """Raw reference rows of valid rays: dict of count, inside0, length, events [n] and t, lo,
        after [n, max_out]."""
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        n = len(rays)
        out = {"count": np.zeros(n, np.uint32), "inside0": np.zeros(n, np.uint32), "length": np.zeros(n, np.float32),
               "events": np.zeros(n, np.uint32), "t": np.zeros((n, max_out), np.float32),
               "lo": np.zeros((n, max_out), np.uint32), "after": np.zeros((n, max_out), np.uint32)}
        if n:
            rc = self.lib.span_ref(ctypes.addressof(self.prog), self.nrec, rays.ctypes.data, n, max_out,
                                   *(out[k].ctypes.data for k in ("count", "inside0", "length", "events", "t", "lo",
                                                                  "after")))
            assert rc == 0
        return out

    def expect(self, rays, max_crossings):
        """(spans[n], crossings[max_crossings, n]) as wo_renderer_trace_spans must give them; crossing
        rows past `stored` hold SENTINEL in every word."""
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        n = len(rays)
        valid = rays_valid(rays)
        safe = rays.copy()
        safe[~valid] = (0, 0, 0, 1, 0, 0, 1, 0)  # the reference takes every ray as valid
        ref = self.reference(safe, max(max_crossings, 1))
        spans = np.zeros(n, dtype=SPANS_DT)
        count = np.where(valid, ref["count"], 0).astype(np.uint32)
        stored = np.minimum(count, max_crossings).astype(np.uint32)
        spans["count"] = count
        spans["stored"] = stored
        spans["length"] = np.where(valid, ref["length"], np.float32(0))
        spans["flags"] = np.where(valid, np.where(ref["inside0"] != 0, wl.RAY_INSIDE, 0)
                                  | np.where(count > stored, wl.RAY_TRUNCATED, 0), wl.RAY_INVALID)
        cross = np.full((max_crossings, n, 4), SENTINEL, dtype=np.uint32).view(CROSSING_DT).reshape(max_crossings, n)
        for k in range(max_crossings):
            on = stored > k
            lo = ref["lo"][on, k]
            leaf = (self.ordpc[lo >> 12] + 1 + (lo & 2047)).astype(np.uint32)
            cross["t"][k, on] = ref["t"][on, k]
            cross["flags"][k, on] = (wl.RAY_HIT | np.where((lo >> 11) & 1, wl.RAY_EXIT, 0)
                                     | np.where(ref["after"][on, k] != 0, wl.RAY_ENTERS, 0))
            cross["leaf"][k, on] = leaf
            cross["node"][k, on] = self.nodes[leaf]
        return spans, cross


def sentinel_crossings(max_crossings, n):
    return np.full((max_crossings, n, 4), SENTINEL, dtype=np.uint32).view(CROSSING_DT).reshape(max_crossings, n)


def same_rows(got, exp, what):
    """Field by field on bits, as test_gpu_rays._same."""
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    bad = {}
    for name in got.dtype.names:
        g = np.ascontiguousarray(got[name]).view(np.uint32).reshape(-1)
        e = np.ascontiguousarray(exp[name]).view(np.uint32).reshape(-1)
        if (g != e).any():
            first = int(np.flatnonzero(g != e)[0])
            bad[name] = (int((g != e).sum()), first, got.reshape(-1)[first], exp.reshape(-1)[first])
    assert not bad, f"{what}: not bit-exact: {bad}"


POINT_SCENES = ["csg256_balanced", "csg256_chain", "csg32", "rtiow_cover", "csg32_nested"]


def sample_points(rec, scene, n=20000):
    """test_marshalling._sample_points of a recorded scene in its SCENE_BOXES box (csg32_nested:
    the box of BOXES), seeded per scene and cast to float32: (m, 3)."""
    import test_marshalling as tm
    lo, hi = (np.array(v, dtype=np.float64) for v in (tm.SCENE_BOXES.get(scene) or BOXES[scene]))
    rng = np.random.default_rng(1000 + POINT_SCENES.index(scene))
    return tm._sample_points(rec, rng, n, lo, hi).astype(np.float32)


def classify_points_f32(prog, nrec, P):
    """The point classification of renderer_ext.h restated in float32 numpy, one rounding per
    operation, BOUND records ignored: bool[n] for (n, 3) float32 points."""
    P = np.asarray(P, dtype=np.float32)
    px, py, pz = P[:, 0], P[:, 1], P[:, 2]
    stack = []
    pc = 0
    while pc < nrec:
        rec = prog[pc]
        if rec.op == wl.WO_OP_BOUND:
            pc += 1
        elif rec.op == wl.WO_OP_PRIM:
            v = np.ones(len(P), dtype=bool)
            for m in range(rec.u0):
                L = prog[pc + 1 + m]
                f = np.array(L.f[:4], dtype=np.float32)
                if L.op == wl.WO_LEAF_SPHERE:
                    gx, gy, gz = px - f[0], py - f[1], pz - f[2]
                    q = (gx * gx + gy * gy) + gz * gz
                else:
                    q = (f[0] * px + f[1] * py) + f[2] * pz
                assert q.dtype == np.float32
                v &= q <= f[3]
            stack.append(v)
            pc += 1 + rec.u0
        else:
            b = stack.pop()
            a = stack.pop()
            stack.append({wl.WO_OP_UNION: a | b, wl.WO_OP_INTER: a & b, wl.WO_OP_DIFF: a & ~b,
                          wl.WO_OP_RDIFF: b & ~a}[rec.op])
            pc += 1
    assert len(stack) == (1 if nrec else 0)
    return stack[0] if stack else np.zeros(len(P), dtype=bool)
