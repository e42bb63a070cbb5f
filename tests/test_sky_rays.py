"""Sky rays (WO_SKY_RAYS): term-mode tracers with a spatial hierarchy state, per lane, when a
ray provably misses the scene (ray_misses_scene, scene_jit.c gen_sky_rays), and
pathtrace_block ends such a path on the sky where it scatters.  Here the generated
predicate is compiled on the host -- its text as generated, with the header's ray
arithmetic (wo_device_common.h between WO_RAY_MATH_BEGIN and WO_RAY_MATH_END) and each
literal-operand instruction restated as the C operation it is -- and held against the
CPU oracle: no ray it accepts has a hit.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle
import test_tile_cull as tc
from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SCENES = ("csg32", "csg32_union")
LEVELS = (1, 2)

_HARNESS = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include "wololo/wo_scene.h"
#define __device__
#define __forceinline__ inline
#define WO_IEEE_SQRT 1   // sqrtf and '/': what sqrt_cr / rcp_cr equal bit for bit (tests/test_gpu_fastmath.py)
#define WO_SPHERE_SKIP 1
#define WO_WK(kind) do { } while (0)
#define WO_WK_N(kind, n) do { } while (0)
#define __builtin_amdgcn_readfirstlane(v) (v)
// a wave of one lane: the wave-level skips then follow this lane's own values
static inline unsigned long long __ballot(bool b) { return b ? 1ull : 0ull; }
static inline float lit(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
namespace wodev {
constexpr float kInf = INFINITY;
@MATH@
}  // namespace wodev

struct Tracer {
@PREDICATE@
};

typedef int (*TraceFn)(const WoRec*, uint32_t, const float*, const float*, float*, uint32_t*, uint32_t*, uint32_t*,
                       uint32_t*);
extern "C" {
// pred[i] = the predicate on ray i; hit[i] = the oracle's answer, t[i] its distance
void sky_check(TraceFn trace, const WoRec* prog, uint32_t n_recs, const float* o, const float* d, uint64_t n,
               uint8_t* pred, uint8_t* hit, float* t) {
    const Tracer tr{};
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i) {
        pred[i] = tr.ray_misses_scene(wodev::f3(o[3 * i], o[3 * i + 1], o[3 * i + 2]),
                                      wodev::f3(d[3 * i], d[3 * i + 1], d[3 * i + 2])) ? 1 : 0;
        uint32_t p, ty, m, ra;
        float tt = INFINITY;
        hit[i] = trace(prog, n_recs, o + 3 * i, d + 3 * i, &tt, &p, &ty, &m, &ra) > 0 ? 1 : 0;
        t[i] = tt;
    }
}
// the hit points of rays (o, d) and their outward unit normals facing the ray, as the path
// tracer's shade forms them; ok[i] = 0 on a miss
void first_hits(TraceFn trace, const WoRec* prog, uint32_t n_recs, const uint32_t* ordpc, const float* o,
                const float* d, uint64_t n, float* P, float* N, uint8_t* ok) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; ++i) {
        uint32_t p = 0, ty = 0, m = 0, ra = 0;
        float t = 0.0f;
        ok[i] = trace(prog, n_recs, o + 3 * i, d + 3 * i, &t, &p, &ty, &m, &ra) > 0 ? 1 : 0;
        if (!ok[i]) continue;
        const WoRec& L = prog[ordpc[p] + 1u + m];
        float q[3], nn[3];
        for (int a = 0; a < 3; ++a) q[a] = o[3 * i + a] + t * d[3 * i + a];
        for (int a = 0; a < 3; ++a) nn[a] = L.op == WO_LEAF_SPHERE ? (q[a] - L.f[a]) * L.f[4] : L.f[a];
        for (int a = 0; a < 3; ++a) {
            P[3 * i + a] = q[a];
            N[3 * i + a] = ty == 0u ? nn[a] : -nn[a];
        }
    }
}
// unit3 of each row, the path tracer's normalisation
void unit_rows(float* v, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        const wodev::F3 u = wodev::unit3(wodev::f3(v[3 * i], v[3 * i + 1], v[3 * i + 2]));
        v[3 * i] = u.x, v[3 * i + 1] = u.y, v[3 * i + 2] = u.z;
    }
}
}
"""

_ASM = (
    (r'asm\("v_sub_f32_e32 %0, 0x([0-9a-f]{8}), %1" : "=v"\((\w+)\) : "v"\(([\w.]+)\)\);', r"\2 = lit(0x\1u) - \3;"),
    (r'asm\("v_subrev_f32_e32 %0, 0x([0-9a-f]{8}), %1" : "=v"\((\w+)\) : "v"\(([\w.]+)\)\);', r"\2 = \3 - lit(0x\1u);"),
    (r'asm\("v_add_f32_e32 %0, 0x([0-9a-f]{8}), %1" : "=v"\((\w+)\) : "v"\(([\w.]+)\)\);', r"\2 = lit(0x\1u) + \3;"),
    (r'asm volatile\("s_mov_b32 %0, 0x([0-9a-f]{8})" : "=s"\((\w+)\)\);', r"\2 = lit(0x\1u);"),
)


def _source(scene):
    r = wl.Renderer("skyrays", max_nodes=4096)
    scenes.build(scene, r)
    src = r.jit_source()
    r.close()
    return src


def _predicates(src):
    """The generated predicates' text (every level, behind its #if)."""
    return src[src.index("// WO_SKY_RAYS_BEGIN"):src.index("// WO_SKY_RAYS_END")].split("\n", 1)[1]


def _level(src, level):
    """One level's function text."""
    parts = re.split(r"#(?:el)?if WO_SKY_RAYS == (\d)\n", _predicates(src))
    text = dict(zip(parts[1::2], parts[2::2]))[str(level)]
    return text.split("#endif")[0]


def _host_text(pred):
    for pat, rep in _ASM:
        pred = re.sub(pat, rep, pred)
    assert "asm" not in pred, re.findall(r".*asm.*", pred)[:3]  # every instruction restated
    return pred


def build_harness(d):
    """Per scene: the host libraries of its predicates by level (built in directory `d`), its
    program, camera and generated source.  (tools/sky_ray_share.py --cpu uses it too.)"""
    prev = os.environ.get("WOLOLO_ALLOW_NO_DEVICE")
    os.environ["WOLOLO_ALLOW_NO_DEVICE"] = "1"  # the generated source only: no device
    try:
        hdr = open(os.path.join(ROOT, "csgrenderer_amd", "csrc", "wo_device_common.h")).read()
        math = hdr[hdr.index("// WO_RAY_MATH_BEGIN"):hdr.index("// WO_RAY_MATH_END")]
        out = {}
        for scene in SCENES:
            r = wl.Renderer("skyrays", max_nodes=4096)
            info = scenes.build(scene, r)
            src = r.jit_source()
            prog, nrec, nprim = r.program()
            fr = r.frame_desc(info.params(width=160, height=90))
            r.close()
            c = d / f"{scene}.cpp"
            c.write_text(_HARNESS.replace("@MATH@", math).replace("@PREDICATE@", _host_text(_predicates(src))))
            libs = {}
            for level in LEVELS:
                so = d / f"{scene}_{level}.so"
                subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fopenmp", "-shared", "-fPIC",
                                f"-DWO_SKY_RAYS={level}", "-I", os.path.join(ROOT, "include"), "-o", str(so), str(c)],
                               check=True)
                libs[level] = ctypes.CDLL(str(so))
            ordpc = np.array([i for i in range(nrec) if prog[i].op == wl.WO_OP_PRIM], dtype=np.uint32)
            out[scene] = dict(libs=libs, prog=prog, nrec=nrec, ordpc=ordpc, cam=fr.cam, src=src)
        return out
    finally:
        if prev is None:
            del os.environ["WOLOLO_ALLOW_NO_DEVICE"]
        else:
            os.environ["WOLOLO_ALLOW_NO_DEVICE"] = prev


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("sky_rays"))


def _trace_fn():
    return ctypes.cast(pyoracle.load().oracle_trace, ctypes.c_void_p)


def _check(s, level, o, d):
    o, d = np.ascontiguousarray(o, dtype=F32), np.ascontiguousarray(d, dtype=F32)
    n = len(o)
    pred, hit, t = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, F32)
    s["libs"][level].sky_check(_trace_fn(), ctypes.c_void_p(ctypes.addressof(s["prog"])), ctypes.c_uint32(s["nrec"]), tc._ptr(o),
                               tc._ptr(d), ctypes.c_uint64(n), tc._ptr(pred), tc._ptr(hit), tc._ptr(t))
    return pred.astype(bool), hit.astype(bool), t


def _unit(s, v):
    v = np.ascontiguousarray(v, dtype=F32)
    s["libs"][1].unit_rows(tc._ptr(v), ctypes.c_uint64(len(v)))
    return v


def _sphere_dirs(rng, n):
    z = rng.uniform(-1.0, 1.0, n)
    a = rng.uniform(0.0, 2.0 * np.pi, n)
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(a), r * np.sin(a), z], axis=1)


def _first_hits(s, o, d):
    n = len(o)
    P, N, ok = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros(n, np.uint8)
    s["libs"][1].first_hits(_trace_fn(), ctypes.c_void_p(ctypes.addressof(s["prog"])), ctypes.c_uint32(s["nrec"]), tc._ptr(s["ordpc"]),
                            tc._ptr(o), tc._ptr(d), ctypes.c_uint64(n), tc._ptr(P), tc._ptr(N), tc._ptr(ok))
    ok = ok.astype(bool)
    return P[ok], N[ok]


def _camera_rays(s, rng, n):
    cam = s["cam"]
    o = np.array(cam.origin[:], dtype=F32)
    ll, hz, vt = (np.array(x[:], dtype=F32) for x in (cam.lower_left, cam.horizontal, cam.vertical))
    sx, ty = rng.uniform(0, 1, (n, 1)).astype(F32), rng.uniform(0, 1, (n, 1)).astype(F32)
    d = ((ll + sx * hz) + ty * vt) - o
    return np.tile(o, (n, 1)), _unit(s, d)


def _scattered(s, rng, n_cam):
    """Lambertian scatters (normal + uniform unit vector, normalised) from the first hits of
    the scene's own camera rays, and from those rays' own first hits in turn."""
    o, d = _camera_rays(s, rng, n_cam)
    outs = []
    for _ in range(2):
        P, N = _first_hits(s, o, d)
        sd = _unit(s, N + _sphere_dirs(rng, len(P)).astype(F32))
        outs.append((P, sd))
        o, d = P, sd
    return np.concatenate([x[0] for x in outs]), np.concatenate([x[1] for x in outs])


def _groups(s):
    """The hierarchy's group spheres and the slab's box, from the tile table."""
    entries = tc._table(s["src"])
    spheres = [(np.array(a), b[0]) for kind, a, b, what in entries if what == "group"]
    boxes = [(np.array(a), np.array(b)) for kind, a, b, what in entries if kind == 2]
    assert len(spheres) >= 2 and len(boxes) == 1
    return spheres, boxes[0]


def _ray_sets(s, rng):
    """{name: (origins, directions)}: at least 200 000 rays in all."""
    sets = {}
    so, sd = _scattered(s, rng, 110_000)
    sets["scattered"] = (so, sd)
    # floor points one ulp above and below the slab's top face (y = 0), and the scattered
    # origins themselves moved one ulp each way
    floor = so[np.abs(so[:, 1]) < 1e-6]
    assert len(floor) > 10_000  # most first hits are on the floor
    up, dn = floor.copy(), floor.copy()
    up[:, 1] = np.nextafter(F32(0), F32(1))
    dn[:, 1] = np.nextafter(F32(0), F32(-1))
    fo = np.concatenate([up, dn, np.nextafter(floor, F32(np.inf)), np.nextafter(floor, F32(-np.inf))])
    fd = _unit(s, np.tile(sd[np.abs(so[:, 1]) < 1e-6], (4, 1)))
    sets["floor +-1 ulp"] = (fo, fd)
    # grazing directions, |d.y| < 1e-6, from floor points (exact, +-1 ulp)
    n = 20_000
    a = rng.uniform(0, 2 * np.pi, n)
    gy = rng.uniform(-1e-6, 1e-6, n)
    gy[: n // 10] = 0.0
    gd = _unit(s, np.stack([np.cos(a), gy, np.sin(a)], axis=1))
    assert (np.abs(gd[:, 1]) < 1e-6).all()
    go = np.concatenate([floor, up, dn])[rng.integers(0, 3 * len(floor), n)]
    sets["grazing"] = (go, gd)
    # from inside each group sphere and the slab's box
    spheres, (lo, hi) = _groups(s)
    io = [c + r * rng.uniform(0, 1, (8_000, 1)) ** (1 / 3) * _sphere_dirs(rng, 8_000) for c, r in spheres]
    io.append(rng.uniform(lo, hi, (8_000, 3)))
    io = np.concatenate(io).astype(F32)
    sets["inside the bounds"] = (io, _sphere_dirs(rng, len(io)).astype(F32))
    # axis-parallel rays and rays with a zero component, from anywhere around the scene
    # and from surface points
    n = 20_000
    ao = np.concatenate([rng.uniform(-8, 8, (n // 2, 3)).astype(F32), so[rng.integers(0, len(so), n // 2)]])
    ad = np.zeros((n, 3), F32)
    ad[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    sets["axis-parallel"] = (ao, ad)
    zd = _sphere_dirs(rng, n)
    zd[np.arange(n), rng.integers(0, 3, n)] = 0.0
    zd[: n // 2, 1] = np.abs(zd[: n // 2, 1])  # half of them leave the floor upwards
    sets["a zero component"] = (ao, _unit(s, zd))
    return sets


@pytest.mark.parametrize("scene", SCENES)
def test_no_accepted_ray_has_a_hit(scene, built):
    s = built[scene]
    sets = _ray_sets(s, np.random.default_rng(20260 + len(scene)))
    total = sum(len(o) for o, _ in sets.values())
    assert total >= 200_000, total
    share = {}
    for level in LEVELS:
        for name, (o, d) in sets.items():
            pred, hit, t = _check(s, level, o, d)
            bad = pred & hit
            assert not bad.any(), (scene, level, name, int(bad.sum()), o[bad][:3], d[bad][:3], t[bad][:3])
            share[level, name] = (float(pred.mean()), float((~hit).mean()))
    print({k: (round(p, 4), round(m, 4)) for k, (p, m) in share.items()})
    # not vacuous: the top-level predicate accepts a fifth of the scattered rays at least
    # (csg32 measured: 32 %), and most of those rays do miss
    assert share[1, "scattered"][0] >= 0.20, share
    assert share[2, "scattered"][0] >= share[1, "scattered"][0]
    # some ray of every set is accepted somewhere, and some has a hit
    for name, (o, d) in sets.items():
        pred, hit, _ = _check(s, 2, o, d)
        assert hit.any(), name
        if name != "inside the bounds":
            assert pred.any(), name


def _consts(text):
    """Bound tests in a piece of generated text: (R^2, cx, cy, cz, R) bit patterns."""
    return re.findall(r's_mov_b32 %0, 0x([0-9a-f]{8})" : "=s"\(bc3\)\);\s*float ox, oy, oz, tca, d2, tr;\s*'
                      r'asm\("v_sub_f32_e32 %0, 0x([0-9a-f]{8}), %1" : "=v"\(ox\).*\n\s*'
                      r'asm\("v_sub_f32_e32 %0, 0x([0-9a-f]{8}), %1" : "=v"\(oy\).*\n\s*'
                      r'asm\("v_sub_f32_e32 %0, 0x([0-9a-f]{8}), %1" : "=v"\(oz\).*\n.*bound_tca_d2.*\n\s*'
                      r'asm\("v_add_f32_e32 %0, 0x([0-9a-f]{8}), %1" : "=v"\(tr\)', text)


def _slab_consts(text):
    """The axis face pairs' offsets in a piece of generated text, in order."""
    return re.findall(r'asm\("v_(sub|add)_f32_e32 %0, 0x([0-9a-f]{8}), %1" : "=v"\(dist[12]\) : "v"\(o\.([xyz])\)\);', text)


@pytest.mark.parametrize("scene", SCENES)
def test_predicate_and_trace_share_their_constants(scene, hostonly):
    src = _source(scene)
    first = src[src.index('WO_MARK("collect_begin")'):src.index('WO_MARK("collect_end")')]
    groups = _consts(first)  # the first pass's group tests, in group order
    assert len(groups) == len(re.findall(r"// group \d+ \(\d+ primitives\)", first)) >= 4
    # the hierarchy as the first pass nests it: group k's children are the groups between
    # it and the end of its block -- here the top groups are 0 and 1, and 1 holds 2 and 3
    l1, l2 = _consts(_level(src, 1)), _consts(_level(src, 2))
    assert l1 == [groups[0], groups[1]]
    assert l2 == [groups[0], groups[2], groups[3]]
    # each group's test in the predicate ends in the trace's own `miss`
    for level in LEVELS:
        text = _level(src, level)
        assert text.count("const bool miss = (d2 > __builtin_fmaf(4e-6f * tca, tca, bc3)) | (tr < 0.0f);") == \
            len(_consts(text))
        assert text.count("gone = gone & miss;") == len(_consts(text))
    # the slab term (outside the hierarchy): the first term of the collect, its box's six
    # faces with the same offsets, and the reach test the trace ballots (csg32) or
    # term_lit states (csg32_union: a one-literal term, gated by term_lit's `valid`)
    slab = first[:first.index("// group 0")]
    assert len(_slab_consts(slab)) == 6
    reach = "!(ia.a > ia.b) & (ia.b > tmin)"
    if scene == "csg32":
        assert f"if (__ballot({reach}) != 0ull)" in slab
    else:
        assert "term_cands1<true>(x, after, best)" in slab
    hdr = open(os.path.join(ROOT, "csgrenderer_amd", "csrc", "wo_device_common.h")).read()
    assert "l.valid = !(iv.a > iv.b) & (iv.b > WO_T_MIN);" in hdr
    for level in LEVELS:
        text = _level(src, level)
        assert _slab_consts(text) == _slab_consts(slab)
        assert text.count(f"gone = gone & !({reach});") == 1
        assert "__ballot" not in text  # a lane's own tests


def test_other_forms_emit_no_predicate(hostonly):
    """BOUND records (csg256_balanced), relevance groups (csg32_nested), a chain's decision
    lists (csg256_chain), and the lane tracer's scenes have no predicate and no switch."""
    for scene in ("csg256_balanced", "csg256_chain", "csg32_nested", "csg360_nested"):
        src = _source(scene)
        assert "ray_misses_scene" not in src and "WO_SKY_RAYS" not in src and "mutable" not in src, scene
    for scene in SCENES:
        src = _source(scene)
        assert src.count("bool ray_misses_scene(wodev::F3 o, wodev::F3 d) const") >= 2
        assert "#ifndef WO_SKY_RAYS\n#define WO_SKY_RAYS " in src
        assert src.index("// WO_SKY_RAYS_BEGIN") > src.index('WO_MARK("collect_end")')  # beside trace, after it
        assert wl.jit_compile_check(src, "gfx950") == ""
