"""Sky rays, level 3 (WO_SKY_RAYS=3, scene_jit.c gen_sky_rays): every group of the hierarchy
opened down to its terms, and each term's first literal tested by one member alone -- the
primitive's sphere through sphere_need, or the face pair of its box's thinnest axis with the
trace's reach condition.  A convex primitive's interval is the meet of its members', so one
member's empty interval empties it.  As tests/test_sky_rays.py does for levels 1 and 2, the
generated predicate is compiled on the host and held against the CPU oracle: no ray it
accepts has a hit, exactly.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_sky_rays as t
from csgrenderer_amd import wololo as wl

F32 = np.float32
LEVEL = 3


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """test_sky_rays's harness (levels 1 and 2), and level 3 from the same translation unit."""
    d = tmp_path_factory.mktemp("sky_rays_terms")
    out = t.build_harness(d)
    for scene, s in out.items():
        so = d / f"{scene}_{LEVEL}.so"
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC",
                        f"-DWO_SKY_RAYS={LEVEL}", "-I", os.path.join(t.ROOT, "include"),
                        "-o", str(so), str(d / f"{scene}.cpp")], check=True)
        s["libs"][LEVEL] = ctypes.CDLL(str(so))
    return out


def _slab_sets(s, rng):
    """Ray sets aimed at the one-pair slab test.  The slab's box from the tile table."""
    _, (lo, hi) = t._groups(s)
    lo, hi = lo.astype(F32), hi.astype(F32)
    ext = hi - lo
    thin = int(np.argmin(ext))
    assert thin == 1 and ext[thin] < 0.1 * min(ext[0], ext[2])  # csg32's slab: 0.5 against 12 x 12
    wide = [a for a in range(3) if a != thin]
    sets = {}
    n = 20_000
    # beside the slab: origins inside its y extent, outside its x / z extent, every direction
    o = rng.uniform(lo - 6.0, hi + 6.0, (n, 3))
    o[:, thin] = rng.uniform(lo[thin], hi[thin], n)
    k = rng.integers(0, 2, n)
    side = np.where(rng.integers(0, 2, n) == 0, lo[wide][k] - rng.uniform(0.01, 6.0, n), hi[wide][k] + rng.uniform(0.01, 6.0, n))
    o[np.arange(n), np.array(wide)[k]] = side
    d = t._sphere_dirs(rng, n)
    d[: n // 4, thin] *= 1e-3  # and nearly level ones, which stay inside the y extent for long
    sets["beside the slab"] = (o.astype(F32), t._unit(s, d))
    # rays that cross the y extent beside the slab: from above and below, aimed past its rim
    o = rng.uniform(lo - 4.0, hi + 4.0, (n, 3))
    o[:, thin] = np.where(rng.integers(0, 2, n) == 0, hi[thin] + rng.uniform(0.0, 3.0, n), lo[thin] - rng.uniform(0.0, 3.0, n))
    to = rng.uniform(lo - 4.0, hi + 4.0, (n, 3))
    to[:, thin] = rng.uniform(lo[thin], hi[thin], n)
    sets["through the y extent"] = (o.astype(F32), t._unit(s, to - o))
    # d.y == 0 at heights inside and outside the slab (on its faces +-1 ulp too)
    a = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(a), np.zeros(n), np.sin(a)], axis=1)
    o = rng.uniform(lo - 3.0, hi + 3.0, (n, 3))
    faces = np.array([lo[thin], hi[thin]], dtype=F32)
    ulps = np.concatenate([faces, np.nextafter(faces, F32(np.inf)), np.nextafter(faces, F32(-np.inf))])
    h = np.concatenate([rng.uniform(lo[thin], hi[thin], n // 4), rng.uniform(hi[thin], hi[thin] + 3.0, n // 4),
                        rng.uniform(lo[thin] - 3.0, lo[thin], n // 4), ulps[rng.integers(0, len(ulps), n - 3 * (n // 4))]])
    o[:, thin] = h
    d = t._unit(s, d)
    assert (d[:, thin] == 0.0).all()
    sets["level rays"] = (o.astype(F32), d)
    # origins on the top and bottom faces +-1 ulp, directions into and out of the slab
    o = rng.uniform(lo - 1.0, hi + 1.0, (n, 3)).astype(F32)
    o[:, thin] = ulps[rng.integers(0, len(ulps), n)]
    d = t._sphere_dirs(rng, n)
    d[: n // 4, thin] *= 1e-4
    sets["on the faces +-1 ulp"] = (o, t._unit(s, d))
    # origins inside the slab
    o = rng.uniform(lo, hi, (n, 3)).astype(F32)
    sets["inside the slab"] = (o, t._sphere_dirs(rng, n).astype(F32))
    return sets


@pytest.mark.parametrize("scene", t.SCENES)
def test_no_accepted_ray_has_a_hit(scene, built):
    s = built[scene]
    rng = np.random.default_rng(3030 + len(scene))
    sets = t._ray_sets(s, rng)
    sets.update(_slab_sets(s, rng))
    share = {}
    for name, (o, d) in sets.items():
        pred, hit, tt = t._check(s, LEVEL, o, d)
        bad = pred & hit
        assert not bad.any(), (scene, name, int(bad.sum()), o[bad][:3], d[bad][:3], tt[bad][:3])
        share[name] = (float(pred.mean()), float((~hit).mean()))
        assert hit.any(), name
    print({k: (round(p, 4), round(m, 4)) for k, (p, m) in share.items()})
    # not vacuous: on the scattered rays level 3 accepts what level 2 does at least, and on
    # each of the slab's sets some ray is accepted -- but on the rays aimed through the y
    # extent beside the slab, which the y pair alone cannot tell from rays that meet it
    # (the price of the single pair; most of them hit something else anyway)
    assert share["through the y extent"][0] == 0.0
    o, d = sets["scattered"]
    p2, p3 = (float(t._check(s, L, o, d)[0].mean()) for L in (2, LEVEL))
    print(f"{scene}: level 2 accepts {100 * p2:.2f} % of the scattered rays, level 3 {100 * p3:.2f} %")
    assert p3 >= p2, (p2, p3)
    for name in ("beside the slab", "level rays", "on the faces +-1 ulp"):
        assert share[name][0] > 0.0, (name, share)


def _spheres(text):
    """Sphere disc tests in a piece of generated text: (cx, cy, cz, r^2) bit patterns."""
    return re.findall(r'asm\("v_subrev_f32_e32 %0, 0x([0-9a-f]{8}), %1" : "=v"\(fx\).*\n\s*'
                      r'asm\("v_subrev_f32_e32 %0, 0x([0-9a-f]{8}), %1" : "=v"\(fy\).*\n\s*'
                      r'asm\("v_subrev_f32_e32 %0, 0x([0-9a-f]{8}), %1" : "=v"\(fz\).*\n.*sphere_fbl.*\n\s*'
                      r'asm\("v_sub_f32_e32 %0, 0x([0-9a-f]{8}), %1" : "=v"\(disc\)', text)


@pytest.mark.parametrize("scene", t.SCENES)
def test_levels_text(scene, hostonly):
    src = t._source(scene)
    first = src[src.index('WO_MARK("collect_begin")'):src.index('WO_MARK("collect_end")')]
    # levels 1 and 2 as they were: the top groups, and group 1's children for it; six faces
    # and three reciprocals
    groups = t._consts(first)
    slab = first[:first.index("// group 0")]
    l1, l2 = t._level(src, 1), t._level(src, 2)
    assert t._consts(l1) == [groups[0], groups[1]] and t._consts(l2) == [groups[0], groups[2], groups[3]]
    for text in (l1, l2):
        assert t._slab_consts(text) == t._slab_consts(slab) and len(t._slab_consts(text)) == 6
        assert text.count("rcp_dir") == 3 and not _spheres(text)
    # level 3: no group is left (each term has a test), one sphere test per term but the
    # slab's, each on constants of the first pass's test of that term, in collect order
    l3 = t._level(src, LEVEL)
    assert not t._consts(l3)
    terms = re.split(r"\{  // term: ", first)[1:]
    assert len(terms) == len(re.findall(r"// tile bit \d+", first)) >= 14
    got = _spheres(l3)
    assert len(got) == len(terms) - 1 == l3.count("gone = gone & !sphere_need(b, disc);")
    for sphere, body in zip(got, terms[1:]):  # (terms[0] is the slab's)
        assert sphere in _spheres(body), (sphere, body[:300])
    if scene == "csg32":
        # ... the first literal's: a lone sphere's only one, the first of `sphere AND NOT
        # sphere`, the sphere member of the box-and-sphere primitive
        assert got == [_spheres(body)[0] for body in terms[1:]]
    # the slab's term keeps the y pair of its six faces -- the trace's constants -- and
    # the trace's reach test
    pairs, six = t._slab_consts(l3), t._slab_consts(slab)
    assert len(pairs) == 2 and pairs == [p for p in six if p[2] == "y"]
    assert l3.count("gone = gone & !(!(ia.a > ia.b) & (ia.b > tmin));") == 1
    assert "__ballot" not in l3 and l3.count("rcp_dir") == 1 and "rcp_dir(d.y)" in l3
    assert "sqrt" not in l3 and "sphere_interval" not in l3


def test_thin_axis_is_derived_from_the_box(hostonly):
    """The pair kept is the one whose planes are closest, whichever axis: a slab standing
    along x keeps its x pair, with its own offsets."""
    from csgrenderer_amd import scenes
    from csgrenderer_amd.wololo import arg
    r = wl.Renderer("thin", max_nodes=256)
    wall, _ = scenes._box_extents(r, (1.0, 0.0, 0.0), (0.25, 6.0, 5.0))
    a = r.union(arg(wall), arg(r.sphere(0.5), (3.0, 1.0, 0.0)))
    r.union(arg(a), arg(r.sphere(0.7), (-3.0, 1.0, 2.0)))
    src = r.jit_source()
    r.close()
    l3 = t._level(src, LEVEL)
    assert [(op, float(np.array(int(h, 16), dtype=np.uint32).view(F32)), ax) for op, h, ax in t._slab_consts(l3)] == \
        [("sub", 1.25, "x"), ("add", -0.75, "x")]
    assert l3.count("rcp_dir") == 1 and "rcp_dir(d.x)" in l3


@pytest.mark.parametrize("scene", t.SCENES)
def test_compiles_without_scratch(scene, hostonly, monkeypatch, capsys):
    """For gfx950 with the runtime's options: no scratch, and the LDS of the kernel without
    the predicate; at most 64 VGPRs, so 8 waves a SIMD."""
    src = t._source(scene)
    monkeypatch.setenv("WOLOLO_JIT_FLAGS", "-DWO_SKY_RAYS=0")
    lds0 = wl.jit_code_resources(src)[1]
    monkeypatch.setenv("WOLOLO_JIT_FLAGS", f"-DWO_SKY_RAYS={LEVEL}")
    assert wl.jit_compile_check(src, "gfx950") == ""
    scratch, lds = wl.jit_code_resources(src)
    assert scratch == 0 and lds == lds0 == (17912 if scene == "csg32" else lds0), (scratch, lds, lds0)
    # the code object's own notes, read as tools/jit_isa.py --rtc reads them
    sys.path.insert(0, os.path.join(t.ROOT, "tools"))
    try:
        import jit_isa
    finally:
        sys.path.pop(0)
    capsys.readouterr()
    assert jit_isa.rtc(src, [f"WO_SKY_RAYS={LEVEL}"], None) == 0
    notes = capsys.readouterr().out
    print(notes)
    vgprs = int(re.search(r"\.vgpr_count:\s*(\d+)", notes).group(1))
    assert vgprs <= 64, notes
    assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", notes).group(1)) == 0, notes
    assert int(re.search(r"\.vgpr_spill_count:\s*(\d+)", notes).group(1)) == 0, notes
    assert "scratch stores: 0 loads: 0" in notes
