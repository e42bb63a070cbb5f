"""Tile pre-cull of the camera-ray waves (wo_device_common.h tile_frustum / tile_culls,
scene_jit.c's bound table): the test the block prologue runs, compiled on the host, never
culls a bound a camera ray of the tile can meet, and the generated source guards every
group and term by its bit.  No GPU."""
import ctypes
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

_HARNESS = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include "wololo/wo_scene.h"
#define __device__
#define __forceinline__ inline
namespace wodev {
constexpr float kInf = INFINITY;
@TILE@
}  // namespace wodev
using namespace wodev;

extern "C" {
// the prologue's test: bit e of out[t] = entry e culled for tile t = (x0, x1, ymin, ymax)
void tile_masks(const WoCamera* cam, float iw, float ih, uint32_t height, const uint32_t* tiles, uint32_t nt,
                const TileBound* tab, uint32_t n, uint64_t* out) {
    for (uint32_t t = 0; t < nt; ++t) {
        TileFrustum tf;
        tile_frustum(*cam, iw, ih, height, tiles[4 * t], tiles[4 * t + 1], tiles[4 * t + 2], tiles[4 * t + 3], tf);
        uint64_t m = 0;
        for (uint32_t e = 0; e < n; ++e)
            if (tile_culls(tf, tab[e])) m |= 1ull << e;
        out[t] = m;
    }
}
// float64: bit e of meet[i] |= ray i (origin o, direction d[i], t >= 0) comes within R of
// entry e's centre, or into its box (touching counts)
void rays_meet(const double* o, const float* d, uint64_t nrays, const TileBound* tab, uint32_t n, uint64_t* meet) {
#pragma omp parallel for
    for (int64_t i = 0; i < (int64_t)nrays; ++i) {
        const double dx = d[3 * i], dy = d[3 * i + 1], dz = d[3 * i + 2], dd = dx * dx + dy * dy + dz * dz;
        uint64_t m = 0;
        for (uint32_t e = 0; e < n; ++e) {
            const TileBound& b = tab[e];
            if (b.kind == 1u) {
                const double cx = b.a[0] - o[0], cy = b.a[1] - o[1], cz = b.a[2] - o[2];
                double t = (cx * dx + cy * dy + cz * dz) / dd;
                if (t < 0.0) t = 0.0;
                const double px = cx - t * dx, py = cy - t * dy, pz = cz - t * dz;
                if (px * px + py * py + pz * pz <= (double)b.b[0] * (double)b.b[0]) m |= 1ull << e;
            } else if (b.kind == 2u) {
                const double dir[3] = {dx, dy, dz};
                double t0 = 0.0, t1 = INFINITY;
                bool hit = true;
                for (int a = 0; a < 3 && hit; ++a) {
                    const double lo = (double)b.a[a] - o[a], hi = (double)b.b[a] - o[a];
                    if (dir[a] == 0.0) {
                        hit = lo <= 0.0 && hi >= 0.0;
                    } else {
                        double ta = lo / dir[a], tb = hi / dir[a];
                        if (ta > tb) { const double s = ta; ta = tb; tb = s; }
                        if (ta > t0) t0 = ta;
                        if (tb < t1) t1 = tb;
                        hit = t0 <= t1;
                    }
                }
                if (hit) m |= 1ull << e;
            }
        }
        meet[i] |= m;
    }
}
// pixels of the tiles that meet an entry their tile culled
uint64_t false_culls(const uint64_t* meet, uint32_t width, const uint32_t* tiles, uint32_t nt, const uint64_t* masks) {
    uint64_t bad = 0;
    for (uint32_t t = 0; t < nt; ++t)
        for (uint32_t y = tiles[4 * t + 2]; y <= tiles[4 * t + 3]; ++y)
            for (uint32_t x = tiles[4 * t]; x < tiles[4 * t + 1]; ++x)
                if (meet[(uint64_t)y * width + x] & masks[t]) ++bad;
    return bad;
}
}
"""


class TileBound(ctypes.Structure):
    _fields_ = [("a", ctypes.c_float * 3), ("b", ctypes.c_float * 3), ("kind", ctypes.c_uint32)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("tile_cull")
    hdr = open(os.path.join(ROOT, "csgrenderer_amd", "csrc", "wo_device_common.h")).read()
    body = hdr[hdr.index("// WO_TILE_CULL_BEGIN"):hdr.index("// WO_TILE_CULL_END")]
    c = d / "tile.cpp"
    c.write_text(_HARNESS.replace("@TILE@", body))
    so = d / "tile.so"
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "include"), "-o", str(so), str(c)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.false_culls.restype = ctypes.c_uint64
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _table(src):
    """The generated source's bound table: [(kind, a, b)] in bit order."""
    m = re.search(r"kTileBound\[(\d+)\] = \{\n(.*?)\n\};", src, re.S)
    rows = re.findall(r"\{\{(\S+), (\S+), (\S+)\}, \{(\S+), (\S+), (\S+)\}, (\d)u\},  // bit (\d+): (group|term) (\d+)", m.group(2))
    assert len(rows) == int(m.group(1))
    out = []
    for i, row in enumerate(rows):
        assert int(row[7]) == i
        v = [float.fromhex(x.rstrip("f")) for x in row[:6]]
        out.append((int(row[6]), v[:3], v[3:], row[8]))
    return out


def _ctable(entries):
    tab = (TileBound * len(entries))()
    for i, e in enumerate(entries):
        tab[i].kind = e[0]
        for k in range(3):
            tab[i].a[k] = e[1][k]
            tab[i].b[k] = e[2][k]
    return tab


@functools.lru_cache(maxsize=None)
def _tiles(width, height):
    """Every workgroup tile a launch can form, as unique (x0, x1, ymin, ymax) of its active
    pixels: 8x8, 8x4 and 4x4 tiles over one rank's rows, and 8x4 / 4x4 tiles over the
    local rows of 3 ranks' 4-row bands (a tile never spans two bands), partial edge tiles
    included."""
    seen = set()
    for tw, th, nranks, tile_rows in [(8, 8, 1, 16), (8, 4, 1, 16), (4, 4, 1, 16), (8, 4, 3, 4), (4, 4, 3, 4)]:
        for rank in range(nranks):
            lrows = wl.local_rows(height, tile_rows, nranks) if nranks > 1 else height
            for ly in range(0, lrows, th):
                rows = [wl.global_row(l, tile_rows, rank, nranks) if nranks > 1 else l for l in range(ly, min(ly + th, lrows))]
                rows = [y for y in rows if y < height]
                if not rows:
                    continue
                assert max(rows) - min(rows) == len(rows) - 1  # one band: contiguous frame rows
                for x0 in range(0, width, tw):
                    seen.add((x0, min(x0 + tw, width), min(rows), max(rows)))
    return np.array(sorted(seen), dtype=np.uint32)


def _job_rays(cam, width, height, iw, ih, jx, jy):
    """job_ray's camera rays of every pixel at jitter (jx, jy), fp32 operation by operation,
    and unit3 of them: (height * width, 3) float32."""
    lx = np.arange(width, dtype=np.uint32).astype(F32)[None, :]
    fy = (np.uint32(height - 1) - np.arange(height, dtype=np.uint32)).astype(F32)[:, None]
    sx = (lx + jx) * iw
    ty = (fy + jy) * ih
    assert sx.dtype == F32 and ty.dtype == F32
    d = []
    for i in range(3):
        ll, hz, vt, og = (F32(cam.lower_left[i]), F32(cam.horizontal[i]), F32(cam.vertical[i]), F32(cam.origin[i]))
        d.append((((ll + sx * hz) + ty * vt) - og) - F32(0.0))
    dot = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    inv = F32(1.0) / np.sqrt(np.maximum(dot, F32(2.0 ** -96)))
    out = np.stack([d[0] * inv, d[1] * inv, d[2] * inv], axis=-1)
    assert out.dtype == F32
    return np.ascontiguousarray(out.reshape(-1, 3))


FRAMES = [(1920, 1080), (61, 35), (17, 5), (1, 1)]
ONE_MINUS = F32(1.0) - F32(2.0 ** -24)


def _check_camera(lib, r, tab, n, width, height, rng, what):
    """Zero false culls for one camera and frame over every tile; returns (culled pairs, pairs)."""
    p = wl.render_params(width, height, spp=1, mode=wl.MODE_PATHTRACE)
    fr = r.frame_desc(p)
    assert fr.cam.lens_radius == 0.0
    tiles = _tiles(width, height)
    masks = np.zeros(len(tiles), dtype=np.uint64)
    lib.tile_masks(ctypes.byref(fr.cam), ctypes.c_float(fr.inv_width), ctypes.c_float(fr.inv_height),
                   ctypes.c_uint32(height), _ptr(tiles), ctypes.c_uint32(len(tiles)), tab, ctypes.c_uint32(n), _ptr(masks))
    meet = np.zeros(width * height, dtype=np.uint64)
    o = np.array([fr.cam.origin[0], fr.cam.origin[1], fr.cam.origin[2]], dtype=np.float64)
    jit = [(F32(0.0), F32(0.0)), (ONE_MINUS, F32(0.0)), (F32(0.0), ONE_MINUS), (ONE_MINUS, ONE_MINUS)]
    for _ in range(2):  # a random jitter per pixel, as the samples have
        jit.append(((rng.integers(0, 1 << 24, (height, width)).astype(F32) * F32(2.0 ** -24)),
                    (rng.integers(0, 1 << 24, (height, width)).astype(F32) * F32(2.0 ** -24))))
    for jx, jy in jit:
        d = _job_rays(fr.cam, width, height, F32(fr.inv_width), F32(fr.inv_height), jx, jy)
        lib.rays_meet(_ptr(o), _ptr(d), ctypes.c_uint64(len(d)), tab, ctypes.c_uint32(n), _ptr(meet))
    bad = lib.false_culls(_ptr(meet), ctypes.c_uint32(width), _ptr(tiles), ctypes.c_uint32(len(tiles)), _ptr(masks))
    assert bad == 0, f"{what} {width}x{height}: {bad} pixels meet a bound their tile culled"
    culled = sum(bin(int(m)).count("1") for m in masks)
    return culled, len(tiles) * n, tiles, masks


def _random_cameras(rng, count, lo, hi):
    cams = []
    for _ in range(count):
        eye = rng.uniform(lo, hi, 3)
        at = rng.uniform(lo, hi, 3)
        if np.linalg.norm(at - eye) < 0.5:
            at = eye + np.array([0.3, -0.4, 1.0])
        cams.append((tuple(eye), tuple(at), float(rng.uniform(10.0, 100.0))))
    return cams


def _cameras_for(entries, rng):
    """Cameras inside spheres and boxes of the table (groups and terms alike), cameras that
    look away from everything, and 20 random ones."""
    cams = []
    for kind, a, b, _ in entries:
        if kind == 1:  # inside the sphere, off its centre, looking across it and away from it
            c, rad = np.array(a), b[0]
            eye = c + rng.uniform(-0.5, 0.5, 3) * rad
            cams.append((tuple(eye), tuple(c + np.array([rad, 0.1 * rad, 0.0])), 60.0))
            cams.append((tuple(eye), tuple(eye + (eye - c) + np.array([0.0, 0.05, 1.0])), 35.0))
        elif kind == 2:
            lo, hi = np.array(a), np.array(b)
            eye = lo + rng.uniform(0.2, 0.8, 3) * (hi - lo)
            cams.append((tuple(eye), tuple(eye + np.array([1.0, 0.4, -0.7])), 70.0))
    return cams


def _scene_cameras(entries, rng):
    inside = _cameras_for(entries, rng)
    away = [((0.0, 30.0, 40.0), (0.0, 60.0, 80.0), 45.0),  # everything behind the camera
            ((0.0, 4.5, 10.0), (0.0, 9.0, 20.0), 45.0),    # csg32's eye, turned round
            ((50.0, 2.0, 0.0), (50.0, 2.0, 10.0), 30.0)]   # everything far off to one side
    return inside, away, _random_cameras(rng, 20, -8.0, 8.0)


def test_tile_cull_never_hides_a_bound_csg32(hostonly, harness):
    """csg32's table (4 groups, 14 terms: spheres and the slab's box): for every tile of
    every frame and camera, no camera ray of the tile -- made as job_ray makes them, fp32
    operation by operation, at jitters 0, 1 - 2^-24 and random -- comes within R of a
    culled sphere's centre or into a culled box (float64).  Also prints the share of
    (tile, entry) pairs culled at 1920x1080 with the scene's camera."""
    r = wl.Renderer("tc", max_nodes=4096)
    scenes.build("csg32", r)
    entries = _table(r.jit_source())
    assert [e[3] for e in entries] == ["group"] * 4 + ["term"] * 14
    assert sorted(e[0] for e in entries) == [1] * 17 + [2]
    tab, n = _ctable(entries), len(entries)
    rng = np.random.default_rng(2024)
    inside, away, rnd = _scene_cameras(entries, rng)
    some_culled = 0
    for width, height in FRAMES:
        culled, pairs, tiles, masks = _check_camera(harness, r, tab, n, width, height, rng, "csg32 own camera")
        if (width, height) == (1920, 1080):
            big = (tiles[:, 1] - tiles[:, 0] == 8) & (tiles[:, 3] - tiles[:, 2] == 7)
            c88 = sum(bin(int(m)).count("1") for m in masks[big])
            allc = int((masks[big] == np.uint64((1 << n) - 1)).sum())
            print(f"\ncsg32 1920x1080, 8x8 tiles: {c88} of {int(big.sum()) * n} (tile, entry) pairs culled "
                  f"({c88 / (int(big.sum()) * n):.4f}); {allc} of {int(big.sum())} tiles cull every entry")
            assert c88 > 0
    # the other cameras: the small frames for all, the full frame for one of each kind
    for label, cams in (("inside", inside), ("away", away), ("random", rnd)):
        for i, (eye, at, fov) in enumerate(cams):
            r.set_camera(eye, at, (0, 1, 0), fov, 0.0, 1.0)
            for width, height in (FRAMES if i < 1 else FRAMES[1:]):
                culled, pairs, _, _ = _check_camera(harness, r, tab, n, width, height, rng, f"csg32 {label} camera {i}")
                some_culled += culled
                if label == "away" and i == 0:
                    assert culled == pairs  # everything lies behind the camera: all culled
    assert some_culled > 0
    r.close()


def test_tile_cull_never_hides_a_bound_synthetic(hostonly, harness):
    """A synthetic table of 64 entries -- tiny and huge spheres, near and far, thin slabs,
    boxes around the origin, entries without a bound -- against cameras inside its
    bounds, looking away, and random ones."""
    rng = np.random.default_rng(77)
    entries = []
    for i in range(64):
        c = rng.uniform(-10.0, 10.0, 3)
        if i % 8 == 7:
            entries.append((0, [0.0] * 3, [0.0] * 3, "term"))
        elif i % 3 == 0:
            h = rng.choice([0.01, 0.3, 2.0, 12.0], 3)
            entries.append((2, list(np.float32(c - h).astype(float)), list(np.float32(c + h).astype(float)), "term"))
        else:
            rad = float(rng.choice([1e-3, 0.05, 0.5, 3.0, 25.0]))
            entries.append((1, list(np.float32(c).astype(float)), [float(np.float32(rad)), 0.0, 0.0], "group"))
    tab, n = _ctable(entries), len(entries)
    r = wl.Renderer("tc", max_nodes=64)
    scenes.build("csg32", r)  # any scene: only the camera is used
    inside = _cameras_for(entries[:24], rng)
    away = [((0.0, 100.0, 0.0), (0.0, 200.0, 1.0), 40.0)]
    total = 0
    for i, (eye, at, fov) in enumerate(inside + away + _random_cameras(rng, 20, -12.0, 12.0)):
        r.set_camera(eye, at, (0, 1, 0), fov, 0.0, 1.0)
        for width, height in (FRAMES if i in (0, 40) else FRAMES[1:]):
            culled, pairs, _, masks = _check_camera(harness, r, tab, n, width, height, rng, f"synthetic camera {i}")
            total += culled
            assert all(not (int(m) >> e) & 1 for m in masks for e in range(7, 64, 8))  # no bound: never culled
    assert total > 0
    r.close()


def test_tile_cull_is_off_with_a_lens(hostonly, harness):
    """aperture > 0: the rays leave a disk, not a point, and nothing is culled."""
    r = wl.Renderer("tc", max_nodes=4096)
    scenes.build("csg32", r)
    entries = _table(r.jit_source())
    tab, n = _ctable(entries), len(entries)
    r.set_camera((0.0, 30.0, 40.0), (0.0, 60.0, 80.0), (0, 1, 0), 45.0, 0.1, 10.0)
    fr = r.frame_desc(wl.render_params(61, 35, spp=1, mode=wl.MODE_PATHTRACE))
    assert fr.cam.lens_radius > 0.0
    tiles = _tiles(61, 35)
    masks = np.ones(len(tiles), dtype=np.uint64)
    harness.tile_masks(ctypes.byref(fr.cam), ctypes.c_float(fr.inv_width), ctypes.c_float(fr.inv_height),
                       ctypes.c_uint32(35), _ptr(tiles), ctypes.c_uint32(len(tiles)), tab, ctypes.c_uint32(n), _ptr(masks))
    assert not masks.any()
    r.close()


def test_generated_source_guards_every_group_and_term(hostonly):
    """csg32's generated source: one table entry per bit of cull[] (the groups' bits, then
    the terms' in collect order), every group's wave-level test behind its bit and its body
    too, every term behind its own, in the first pass and in the re-collect; trace starts
    from the tracer's `pre` words and returns at once when all are set.  The scenes whose
    tracer is not in term mode have no table (their kernels are as before)."""
    r = wl.Renderer("tc", max_nodes=4096)
    scenes.build("csg32", r)
    src = r.jit_source()
    r.close()
    entries = _table(src)
    ngroups = sum(1 for e in entries if e[3] == "group")
    nterms = len(entries) - ngroups
    m = re.search(r"kTileCullEntries = (\d+)u, kTileCullWords = (\d+)u;", src)
    assert int(m.group(1)) == len(entries) and int(m.group(2)) == (len(entries) + 31) // 32
    assert int(re.search(r"// term mode: (\d+) terms", src).group(1)) == nterms
    lines = src.splitlines()
    end1 = next(i for i, l in enumerate(lines) if 'WO_MARK("collect_end")' in l)
    first, second = lines[:end1], lines[end1:]
    for name, part in (("first pass", first), ("re-collect", second)):
        bits = []
        for i, l in enumerate(part):
            if "// term:" in l:
                g = re.fullmatch(r"\s*if \(!\(cull\[(\d+)\] & (\d+)u\)\) \{  // tile bit (\d+)", part[i - 1])
                assert g, (name, part[i - 1])
                k = int(g.group(3))
                assert int(g.group(1)) == k // 32 and int(g.group(2)) == 1 << (k % 32)
                bits.append(k)
        assert bits == list(range(ngroups, ngroups + nterms)), (name, bits)
    seen = []
    for i, l in enumerate(first):
        g = re.search(r"// group (\d+) \((\d+) primitives\)", l)
        if not g:
            continue
        k = int(g.group(1))
        seen.append(k)
        guard = f"(cull[{k // 32}] & {1 << (k % 32)}u)"
        assert first[i + 1].strip() == f"if ({guard} == 0u) {{"  # the test runs only when the bit is not set on entry
        j = next(j for j in range(i + 1, len(first)) if first[j].strip().startswith("if (!(cull["))
        assert first[j].strip() == f"if (!{guard}) {{"
        assert "__ballot(!miss)" in "\n".join(first[i:j])
    assert seen == list(range(ngroups))
    for k in range(ngroups):  # the re-collect honours the groups' bits too
        assert any(l.strip() == f"if (!(cull[{k // 32}] & {1 << (k % 32)}u)) {{" for l in second)
    full = (1 << len(entries)) - 1
    assert f"if ((pre[0] == 0x{full & 0xffffffff:08x}u)) return false;" in src
    assert src.index("return false;") < src.index("wodev::rcp_dir(")  # before any arithmetic
    assert "cull[0] = pre[0];" in src
    for other in ("csg256_balanced", "csg256_chain", "csg32_nested"):
        r = wl.Renderer("tc", max_nodes=4096)
        scenes.build(other, r)
        assert "kTileBound" not in r.jit_source() and "pre[" not in r.jit_source(), other
        r.close()


def test_tile_table_bounds_csg32_terms(hostonly):
    """The table's term entries are the bounds DESIGN 3.5 states: a term's smallest positive
    literal's smallest sphere, and for the slab-minus-crater term (no sphere in its positive
    literal) the slab's box from its axis half-spaces."""
    r = wl.Renderer("tc", max_nodes=4096)
    scenes.build("csg32", r)
    src = r.jit_source()
    prog, nrec, _ = r.program()
    r.close()
    entries = _table(src)
    terms = [e for e in entries if e[3] == "term"]
    pc_of = {prog[i].u1: i for i in range(nrec) if prog[i].op == wl.WO_OP_PRIM}
    first = src[:src.index('WO_MARK("collect_end")')]
    found = re.findall(r"// term: (NOT )?primitive (\d+)(?: AND (NOT )?primitive (\d+))?", first)
    assert len(found) == len(terms)
    for (n0, o0, n1, o1), (kind, a, b, _) in zip(found, terms):
        pos = [int(o) for neg, o in ((n0, o0), (n1, o1)) if o and not neg]
        leaves = [prog[pc_of[o] + 1 + m] for o in pos for m in range(prog[pc_of[o]].u0)]
        spheres = [L for L in leaves if L.op == wl.WO_LEAF_SPHERE]
        if spheres:
            L = min(spheres, key=lambda L: L.f[3])
            assert kind == 1 and a == [L.f[0], L.f[1], L.f[2]]
            assert b[0] == float(np.float32(math.sqrt(L.f[3])))
        else:
            assert kind == 2 and a == [-6.0, -0.5, -6.0] and b == [6.0, 0.0, 6.0]
