"""Shared by tests/test_features.py and tests/test_gpu_features.py (test helper, no fixture): the
CPU reference of the first-hit feature buffers (tests/host/feature_ref.c over the oracle's own
functions) and the planes, whole frames and rank buffers it expects."""
import ctypes
import os
import subprocess

import numpy as np

from csgrenderer_amd import wololo as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS_DT = np.dtype(wl.FEATURE_IDS_FIELDS)
MISS_IDS = (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0)
SENTINEL = 0xA5A5A5A5  # every word of a row the query must not write


def build_feature_ref(outdir):
    """Compile tests/host/feature_ref.c with span_support.build_span_ref's flags (the oracle
    Makefile's); the loaded library."""
    so = os.path.join(str(outdir), "feature_ref.so")
    subprocess.run(["gcc", "-std=c11", "-O2", "-mfma", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                    "-fno-unsafe-math-optimizations", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "oracle"), "-shared", "-o", so,
                    os.path.join(ROOT, "tests", "host", "feature_ref.c"), "-lm"], check=True)
    lib = ctypes.CDLL(so)
    lib.feature_ref.restype = ctypes.c_int
    lib.feature_ref.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32] + \
        [ctypes.c_void_p] * 5
    return lib


def params(w, h, spp, seed=9, sample_offset=5, max_depth=8):
    return wl.render_params(w, h, spp=spp, max_depth=max_depth, seed=seed, mode=wl.MODE_PATHTRACE,
                            sample_offset=sample_offset)


class FeatureScene:
    """A compiled scene, its materials and camera as the reference needs them."""

    def __init__(self, lib, r):
        self.lib, self.r = lib, r
        self.prog, self.nrec, self.nprims = r.program()
        self.mats, self.n_mats = r.materials()
        self.nodes = np.ascontiguousarray(r.program_nodes(), dtype=np.uint32)
        if not len(self.nodes):
            self.nodes = np.zeros(1, dtype=np.uint32)

    def pixels(self, p, xs, ys):
        """The reference's values at pixels (xs, ys) of the frame p: dict of albedo, normal [n, 4]
        float32, ids [n] IDS_DT, hits [n] and the raw sums [n, 7] (albedo rgb, normal xyz, t)."""
        xs = np.ascontiguousarray(xs, dtype=np.uint32)
        ys = np.ascontiguousarray(ys, dtype=np.uint32)
        n = len(xs)
        fr = self.r.frame_desc(p, 16, 0, 1)
        out = {"albedo": np.zeros((n, 4), np.float32), "normal": np.zeros((n, 4), np.float32),
               "ids": np.zeros((n, 4), np.uint32), "hits": np.zeros(n, np.uint32), "sums": np.zeros((n, 7), np.int64)}
        rc = self.lib.feature_ref(ctypes.addressof(self.prog), self.nrec, ctypes.addressof(self.mats), self.n_mats,
                                  self.nodes.ctypes.data, ctypes.addressof(fr), xs.ctypes.data, ys.ctypes.data, n,
                                  *(out[k].ctypes.data for k in ("albedo", "normal", "ids", "hits", "sums")))
        assert rc == 0
        out["ids"] = out["ids"].view(IDS_DT).reshape(n)
        return out

    def frame(self, p):
        """The three planes of the whole frame: (albedo (H, W, 4), normal (H, W, 4), ids (H, W)) and
        the hit counts (H, W).  Read-only, to be shared between tests."""
        h, w = p.height, p.width
        ys, xs = np.divmod(np.arange(h * w, dtype=np.uint32), np.uint32(w))
        ref = self.pixels(p, xs, ys)
        planes = (ref["albedo"].reshape(h, w, 4), ref["normal"].reshape(h, w, 4), ref["ids"].reshape(h, w),
                  ref["hits"].reshape(h, w))
        for a in planes:
            a.setflags(write=False)
        return planes


def as_words(plane):
    """A plane (float32 (..., 4) or IDS_DT (...)) as its uint32 words (..., 4)."""
    a = np.ascontiguousarray(plane)
    if a.dtype == IDS_DT:
        return a.view(np.uint32).reshape(a.shape + (4,))
    return a.view(np.uint32)


def rank_buffer(planes, p, tile_rows, rank, nranks, band=(0, 0), plane_stride=None):
    """What render_features_device leaves in a buffer of 3 * plane_stride rows filled with SENTINEL:
    uint32 (3 * plane_stride, 4).  Local rows past the frame's last row keep the sentinel."""
    rows = wl.local_rows(p.height, tile_rows, nranks, band)
    stride = rows * p.width if plane_stride is None else plane_stride
    buf = np.full((3 * stride, 4), SENTINEL, dtype=np.uint32)
    for k in range(3):
        words = as_words(planes[k])
        for lrow in range(rows):
            y = wl.global_row(lrow, tile_rows, rank, nranks, band)
            if y < p.height:
                at = k * stride + lrow * p.width
                buf[at:at + p.width] = words[y]
    return buf


def same_planes(got, exp, what):
    """Three planes against three planes, every word."""
    names = ("albedo", "normal", "ids")
    for k in range(3):
        g, e = as_words(got[k]), as_words(exp[k])
        assert g.shape == e.shape, (what, names[k], g.shape, e.shape)
        bad = (g != e).any(axis=-1)
        if bad.any():
            first = tuple(int(v) for v in np.argwhere(bad)[0])
            raise AssertionError(f"{what}: plane {names[k]} not bit-exact at {int(bad.sum())} pixels, first {first}: "
                                 f"got {got[k][first]}, expected {exp[k][first]}")


def same_words(got, exp, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = (got != exp).any(axis=-1)
    if bad.any():
        first = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} rows differ, first row {first}: got {got[first]}, "
                             f"expected {exp[first]}")


def blacken(r):
    """Give every sphere / half-space node of the scene a black Lambertian material."""
    black = r.lambertian((0.0, 0.0, 0.0))
    leaves = sorted({int(n) for n in r.program_nodes() if n != wl.WO_NODE_INVALID})
    assert leaves
    for n in leaves:
        r.set_material(n, black)
    return black
