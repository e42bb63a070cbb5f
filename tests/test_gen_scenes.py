"""Generated CSG scenes at every kernel-form boundary: the case table, checked on the CPU.

scene_jit.c and lane_bvh_build.cpp pick a code shape from the structure of the tree.
`CASES` lists seeded scenes (tests/gen_scenes.py) that land on each shape; what a row is
*for* is a set of facts this file asserts from the generated source, the compiled program
and the lane BVH descriptor, so a change of generator, seed or size that moves a row off its
form fails here, before the GPU file (tests/test_gpu_gen_scenes.py) renders the rows.

Per row, on the oracle alone: the frame is telling (enough camera rays hit, enough bounces),
the oracle's hits lie where an independent float64 point classifier changes membership, the
generated source compiles for gfx950 and its root evaluation, compiled on the host, is the
program's value.
"""
import re
import time
from collections import namedtuple

import numpy as np
import pytest

import gen_scenes as gs
import pyoracle
from csgrenderer_amd import wololo as wl
from test_jit import _check_generated_eval
from test_scene_compile import _program_checks

Case = namedtuple("Case", "name family n seed knobs cam want")
W, H = 48, 36  # the frame of every row: the width no multiple of 64, the height none of 8
# telling conditions (on the inputs, judged on the oracle): the share of camera rays that
# hit, segments per sample of the path-trace frame, camera rays through a coincident pair
HIT_SHARE, SEGS_PER_SAMPLE, TIE_SHARE = (0.15, 0.9), 1.3, 0.05


def _c(name, family, n, seed, cam, knobs=None, **want):
    return Case(name, family, n, seed, knobs or {}, cam, want)


GENERAL = {"terms": 0, "general": 1, "union_only": 0, "kind": 7}
# want: forms (the set of markers of gen_scenes.MARKERS, "flat" for none), nprim (a count
# or a range), words, lds_prog, hbits_lds, window, lut_subtrees, rdiff / bound (records of
# that kind present), lane (fields of the descriptor and the kernel kind), ties
CASES = [
    # flat root evaluation (no marker, the 5-event register window): the default of any mid-size tree
    _c("flat_w1", "chain", 34, 1, ((-0.48, 0.72, 4.78), (-0.48, 0.25, 0.52), 40.0),
       forms={"flat"}, nprim=(24, 32), words=1, window=5, lds_prog=1, lane=dict(GENERAL, gwords=2)),
    _c("flat_w2", "random", 50, 3, ((-0.11, 0.16, 6.09), (-0.11, -0.43, 0.74), 40.0),
       forms={"flat"}, nprim=(33, 64), words=2, window=5, lds_prog=1, bound=True, lane=dict(GENERAL, gwords=3)),
    # ... on both sides of the 6 KB switch between the program in LDS and in global memory
    _c("flat_lds_prog", "balanced", 50, 3, ((-0.86, 1.65, 6.79), (-0.86, 0.67, 0.09), 40.0),
       forms={"flat"}, nprim=(33, 64), words=2, window=5, lds_prog=1, rdiff=True, lane=dict(GENERAL, gwords=3)),
    _c("flat_global_prog", "balanced", 70, 2, ((-0.22, 0.81, 5.04), (-0.22, 0.43, 2.39), 40.0),
       forms={"flat"}, nprim=(33, 64), words=2, window=5, lds_prog=0, rdiff=True, lane=dict(GENERAL, gwords=4)),
    # decision lists and truth tables in one kernel
    _c("dl_lut", "balanced", 34, 1, ((-0.52, 1.46, 5.77), (-0.52, 0.99, 1.38), 40.0),
       forms={"dl", "lut"}, nprim=(13, 36), words=1, window=8, lut_subtrees=3, lane=GENERAL),
    _c("dl_lut_small", "random", 14, 1, ((1.15, -0.16, 5.11), (1.15, -0.54, 1.61), 40.0),
       forms={"dl", "lut"}, nprim=12, words=1, window=8, lut_subtrees=1, lane=GENERAL),
    # truth tables under a root that is a union of conjunctions, one of them of more than two
    # literals ((a \\ b) \\ c): too long for the lanes' term mode, which must leave it to their
    # general form (the builder once kept the rejected terms and wrote term records for them)
    _c("lut_long_term", "balanced", 14, 1, ((-0.79, 1.52, 4.86), (-0.79, 0.91, -0.7), 40.0),
       forms={"lut"}, nprim=14, words=1, window=8, lut_subtrees=2, lane=dict(GENERAL, gwords=1)),
    # decision lists over two words, with RDIFF records
    _c("dl_w2_rdiff", "random", 50, 11, ((1.19, -0.32, 5.92), (1.19, -0.88, 0.87), 40.0),
       forms={"dl"}, nprim=(33, 64), words=2, window=5, rdiff=True, lane=dict(GENERAL, gwords=3)),
    # levelled tables, the membership words in registers (fewer than 4 words) ...
    _c("hlut_regs", "balanced", 90, 3, ((-0.08, 0.99, 3.58), (-0.08, 0.63, 0.33), 40.0),
       forms={"hlut"}, nprim=(65, 96), words=3, window=14, hbits_lds=0, lds_prog=0, rdiff=True,
       lane=dict(GENERAL, gwords=5)),
    _c("hlut_regs_random", "random", 90, 3, ((2.22, -1.26, 2.33), (2.22, -1.51, 0.0), 40.0),
       forms={"hlut"}, nprim=(65, 96), words=3, window=14, hbits_lds=0, rdiff=True, lane=dict(GENERAL, gwords=5)),
    # ... and in LDS at exactly 4 words
    _c("hlut_4w", "balanced", 120, 1, ((-1.25, 2.89, 4.85), (-1.25, 2.62, 2.96), 40.0),
       forms={"hlut"}, nprim=(97, 128), words=4, window=14, hbits_lds=1, rdiff=True, lane=dict(GENERAL, gwords=7)),
    # term mode across the word boundary (exact pairs: primitives == leaves)
    _c("term_33", "pairs", 33, 1, ((-1.03, -0.33, 8.96), (-1.03, -1.26, 0.39), 40.0), {"exact": True},
       forms={"term"}, nprim=33, words=2, lds_prog=1, lane={"terms": 25, "general": 0, "union_only": 0, "kind": 6}),
    _c("term_64", "pairs", 64, 1, ((0.49, 0.91, 9.74), (0.49, -0.33, 1.26), 40.0), {"exact": True},
       forms={"term"}, nprim=64, words=2, lds_prog=0, lane={"terms": 48, "general": 0, "union_only": 0, "kind": 6}),
    # one primitive past term mode's limit: the incremental union count takes over
    _c("pairs_65", "pairs", 65, 1, ((-0.82, 3.59, 11.46), (-0.82, 2.59, 2.3), 40.0), {"exact": True},
       forms={"ucount"}, nprim=65, words=3, lds_prog=0, lane={"terms": 49, "general": 0, "union_only": 0, "kind": 6}),
    _c("ucount_95", "pairs", 120, 1, ((0.15, 2.28, 15.46), (0.15, 0.81, 2.02), 40.0),
       forms={"ucount"}, nprim=(80, 130), words=3, lane={"terms": 73, "general": 0, "union_only": 0, "kind": 6}),
    # union / difference chains of spheres: one decision list, at and across the word boundary
    _c("chain_32", "chain", 32, 1, ((-0.12, 1.17, 6.42), (-0.12, 0.59, 1.11), 40.0),
       {"halfspaces": 0, "ops": (0.6, 0, 0.4)}, forms={"dl"}, nprim=32, words=1, lane=dict(GENERAL, gwords=2)),
    _c("chain_33", "chain", 33, 1, ((-0.33, 0.92, 5.55), (-0.33, 0.35, 0.35), 40.0),
       {"halfspaces": 0, "ops": (0.6, 0, 0.4)}, forms={"dl"}, nprim=33, words=2, lane=dict(GENERAL, gwords=3)),
    _c("one_prim", "random", 1, 1, ((0.0, 0.3, 2.9), (0.0, 0.0, 0.63), 40.0),
       forms={"term"}, nprim=1, words=1, lds_prog=1,
       lane={"terms": 0, "general": 0, "union_only": 1, "spheres_only": 1, "kind": 3}),
    # coincident and tangent surfaces (equal event keys) in term mode, under the union count
    # and, folded with differences and intersections, in an event-list form (4 truth tables:
    # the largest split lut_plan takes)
    _c("ties_term", "ties", 0, 2, ((-0.39, 0.51, 5.78), (-0.39, -0.28, 0.39), 40.0),
       forms={"term"}, nprim=14, words=1, ties=True, lane={"terms": 12, "general": 0, "union_only": 0, "kind": 6}),
    _c("ties_ucount", "ties", 0, 1, ((0.15, 1.35, 9.52), (0.15, 0.25, -0.52), 40.0), {"extra": 30},
       forms={"ucount"}, nprim=74, words=3, ties=True, lane={"terms": 57, "general": 0, "union_only": 0, "kind": 6}),
    _c("ties_nest", "ties", 0, 2, ((0.08, 0.69, 5.28), (0.08, 0.1, 1.21), 40.0), {"nest": True},
       forms={"lut"}, nprim=19, words=1, window=8, lut_subtrees=4, rdiff=True, ties=True, lane=dict(GENERAL, gwords=2)),
    # a DAG (three operands used twice) with three roots: the scene is their balanced union
    _c("dag_3_roots", "random", 60, 4, ((0.13, 0.66, 2.4), (0.13, 0.39, -0.1), 40.0), {"roots": 3, "reuse": 3},
       forms={"flat"}, nprim=(33, 64), words=2, rdiff=True, roots=3, lane=dict(GENERAL, gwords=4)),
    # union-only over generic primitives (spheres cut by half-spaces): the lanes' binary walk,
    # and a second lane scene for the ray queries
    _c("union_generic", "balanced", 40, 1, ((0.44, 1.32, 9.93), (0.44, 0.37, 1.23), 40.0),
       {"ops": (1, 0, 0), "carve": 0, "halfspaces": 0.5}, forms={"term"}, nprim=(24, 32), words=1,
       lane={"terms": 0, "general": 0, "union_only": 1, "spheres_only": 0, "kind": 2}),
]
BY_NAME = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
EVENT_LIST = [c.name for c in CASES if "term" not in c.want["forms"]]


def make(case, tracer=None):
    """The row's scene in a new renderer with its camera set: (renderer, Shadow)."""
    r = wl.Renderer(case.name, max_nodes=4096)
    sh = gs.build(r, case.family, case.n, case.seed, **case.knobs)
    look_from, look_at, vfov = case.cam
    r.set_camera(look_from, look_at, (0, 1, 0), vfov)
    if tracer:
        r.set_tracer(tracer)
    return r, sh


def frame_params(mode):
    return wl.render_params(W, H, spp=4 if mode == wl.MODE_PATHTRACE else 1, max_depth=6, mode=mode, seed=7)


def check_facts(case, d):
    """`d` (gen_scenes.describe, or the same facts read from a rendered source) is what the row claims."""
    want = case.want
    for key, v in want.items():
        if key in ("ties", "roots"):
            continue
        if key == "nprim" and isinstance(v, tuple):
            assert v[0] <= d["nprim"] <= v[1], (case.name, key, d["nprim"])
        elif key in ("rdiff", "bound"):
            assert (d[key] > 0) == v, (case.name, key, d[key])
        elif key == "lane":
            assert {k: d["lane"][k] for k in v} == v, (case.name, d["lane"])
        else:
            assert d[key] == v, (case.name, key, d[key])
    if d["forms"] == {"flat"}:
        assert d["window"] == 5, (case.name, d["window"])


def coincident_spheres(prog, nrec):
    """Sphere leaf records that share the bits of f[0:4] with another one: {bits: [pc, ...]}."""
    seen = {}
    for pc in range(nrec):
        if prog[pc].op == wl.WO_LEAF_SPHERE:
            seen.setdefault(np.array(prog[pc].f[:4], dtype=np.float32).tobytes(), []).append(pc)
    return {k: v for k, v in seen.items() if len(v) >= 2}


def _camera_rays(r):
    p = frame_params(wl.MODE_NORMALS)
    return [r.pixel_ray(p, x, y) for y in range(H) for x in range(W)]


@pytest.mark.parametrize("name", NAMES)
def test_row_is_the_form_it_claims(hostonly, name):
    case = BY_NAME[name]
    r, sh = make(case)
    prog, nrec, nprim = r.program()
    _program_checks(prog, nrec, nprim)
    d = gs.describe(r)
    print(name, d)
    check_facts(case, d)
    assert len(sh.roots()) == case.want.get("roots", 1)
    if case.knobs.get("reuse") or case.family == "ties":
        # a DAG: some node is an operand in two places
        used = [a.node for nd in sh.nodes if nd[0] in "uid" for a in nd[1:3]]
        assert len(used) > len(set(used))
    assert not sh.scene_inside(np.array(case.cam[0], dtype=np.float64)), "the camera is inside the solid"
    r.close()


def test_every_form_has_a_row():
    got = {frozenset(c.want["forms"]) for c in CASES}
    assert got >= {frozenset(f) for f in ({"flat"}, {"dl"}, {"lut"}, {"dl", "lut"}, {"hlut"}, {"term"}, {"ucount"})}
    assert {c.want["lane"]["kind"] for c in CASES} >= {2, 3, 6, 7}


@pytest.mark.parametrize("name", NAMES)
def test_row_is_telling(hostonly, name):
    case = BY_NAME[name]
    r, _ = make(case)
    prog, nrec, _ = r.program()
    mats, nm = r.materials()
    rays = _camera_rays(r)
    hit = np.array([pyoracle.trace(prog, nrec, ray[0:3], ray[4:7]) is not None for ray in rays])
    p = frame_params(wl.MODE_PATHTRACE)
    img, segs = pyoracle.pathtrace_rows(prog, nrec, mats, nm, r.frame_desc(p), 0, H)
    print(name, "hit share", hit.mean(), "segments per sample", segs / (W * H * p.spp))
    assert np.isfinite(img).all()
    assert HIT_SHARE[0] <= hit.mean() <= HIT_SHARE[1]
    assert segs / (W * H * p.spp) >= SEGS_PER_SAMPLE
    if case.want.get("ties"):
        # coincidence is structural (two leaf records, the same bits), and the camera sees it:
        # each coincident sphere alone, as a two-leaf scene under the row's camera
        pairs = coincident_spheres(prog, nrec)
        assert len(pairs) >= 2
        crossed = np.zeros(len(rays), dtype=bool)
        for key in pairs:
            cx, cy, cz, rr = (float(v) for v in np.frombuffer(key, dtype=np.float32))
            r2 = wl.Renderer("pair", max_nodes=8)
            s = r2.sphere(float(np.sqrt(rr)))
            r2.union(wl.arg(s, (cx, cy, cz)), wl.arg(s, (cx, cy, cz)))
            p2, n2, _ = r2.program()
            crossed |= np.array([pyoracle.trace(p2, n2, ray[0:3], ray[4:7]) is not None for ray in rays])
            r2.close()
        print(name, "rays through a coincident pair", crossed.mean())
        assert crossed.mean() >= TIE_SHARE
    r.close()


def classifier_agrees(sh, o, d, t, root_after):
    """A hit at t on the ray o + t d against the float64 classifier: None when another
    boundary lies within eps (membership equal on both sides: ambiguous), else whether the
    classifier's membership behind the hit is `root_after`."""
    eps = 2e-4 * max(1.0, t)
    before, after = sh.scene_inside_many([o + (t - eps) * d, o + (t + eps) * d])
    if before == after:
        return None
    return bool(after) == bool(root_after)


@pytest.mark.parametrize("name", NAMES)
def test_hits_match_float64_classifier(hostonly, name):
    """test_scene_compile's check of the oracle against the float64 point classifier, over
    60 rays of each row (and rays aimed at points inside the solid)."""
    case = BY_NAME[name]
    r, sh = make(case)
    prog, nrec, nprim = r.program()
    rng = np.random.default_rng(1000 + case.seed)
    # the vectorised classifier is the scalar one
    pts = np.array(case.cam[1]) + rng.uniform(-2.5, 2.5, (40, 3))
    assert [sh.scene_inside(p) for p in pts] == list(sh.scene_inside_many(pts))
    tied = {pc for pcs in coincident_spheres(prog, nrec).values() for pc in pcs} if case.want.get("ties") else set()
    ordpc = {prog[pc].u1: pc for pc in range(nrec) if prog[pc].op == wl.WO_OP_PRIM}
    look_from, look_at = (np.array(v, dtype=np.float64) for v in case.cam[:2])
    n_all = n_hit = n_checked = 0
    tmin = wl.WO_T_MIN
    # origins around the camera and targets around the look-at point, both spread over about
    # what the camera sees (a 40 degree field of view: half its distance is a little more)
    spread = 0.5 * np.linalg.norm(look_from - look_at)
    for _ in range(60):
        o = look_from + rng.uniform(-spread, spread, 3)
        d = look_at + rng.uniform(-spread, spread, 3) - o
        d = (d / np.linalg.norm(d)).astype(np.float32)
        o = o.astype(np.float32)
        of, df = o.astype(np.float64), d.astype(np.float64)
        res = pyoracle.trace(prog, nrec, o.tolist(), d.tolist())
        if res is None:
            ts = np.linspace(tmin + 1e-3, 30.0, 400)
            vals = sh.scene_inside_many(of + ts[:, None] * df)
            assert len(set(vals.tolist())) == 1, (name, "missed boundary")
            continue
        t, prim, typ, member, root_after = res
        n_all += 1
        eps = 2e-4 * max(1.0, t)
        # at a coincident surface the hit is decided by the key order, which the classifier
        # has no say in (both sides of a \ a' are outside): the before / after probe is not
        # made there, and the hit does not count for the cap; the rest of the check is
        if ordpc[prim] + 1 + member not in tied:
            n_hit += 1
            ok = classifier_agrees(sh, of, df, t, root_after)
            if ok is not None:
                n_checked += 1
                assert ok, (name, t)
            else:
                continue
        # nothing changes between tmin and the hit
        ts = np.linspace(tmin + eps, t - eps, 64)
        vals = sh.scene_inside_many(of + ts[:, None] * df)
        assert len(set(vals.tolist())) == 1, (name, t)
    print(name, "hits", n_all, "off coincident surfaces", n_hit, "checked", n_checked)
    assert n_all >= 10 and n_checked >= n_hit * 0.8
    pts = look_at + np.random.default_rng(case.seed).uniform(-4, 4, (3000, 3))
    for p in pts[sh.scene_inside_many(pts)][:20]:
        o = look_from + rng.uniform(-1, 1, 3)
        if sh.scene_inside(o):
            continue
        d = p - o
        dist = np.linalg.norm(d)
        d = (d / dist).astype(np.float32)
        res = pyoracle.trace(prog, nrec, o.astype(np.float32).tolist(), d.tolist())
        assert res is not None and res[0] <= dist * (1 + 1e-4) + 1e-4, (name, p, res)
    r.close()


@pytest.mark.parametrize("name", NAMES)
def test_generated_source_compiles_and_evaluates(hostonly, tmp_path, name):
    case = BY_NAME[name]
    r, _ = make(case)
    prog, nrec, nprim = r.program()
    src = r.jit_source()
    r.close()
    t0 = time.perf_counter()
    assert wl.jit_compile_check(src, "gfx950") == ""
    print(name, f"{len(src)} B of source, hiprtc {time.perf_counter() - t0:.1f} s")
    if name in EVENT_LIST:
        assert "WO_EVAL_BEGIN" in src
        forms = gs.forms(src)
        if "// relevance group" in src:
            # the relevance groups number cull[]'s bits and a set bit means "cannot change the
            # root", so no root evaluation may read one as a BOUND record's "this subtree is
            # false" (the WO_JIT_LUT=0 evaluation once did; the host harness, which leaves
            # cull[] at 0, cannot see that)
            # (every root evaluation: the marked block, and the copies the sweep makes of it, which
            # all sit under `#if WO_JIT_LUT` ... `#else` ... `#endif`)
            marked = src[src.index("// WO_EVAL_BEGIN"):src.index("// WO_EVAL_END")].split("\n", 1)[1]
            assert "bits[" in marked and "cull[" not in marked
            if "lut" in forms:
                blocks = re.findall(r"^#if WO_JIT_LUT\n(.*?)^#endif", src, re.S | re.M)
                flat = [b.split("#else\n", 1)[1] for b in blocks if "uint32_t lsub" in b]
                assert len(flat) >= 2 and any(b in marked for b in flat), len(flat)
                for b in flat:
                    assert "bits[" in b and "cull[" not in b
        for lut in ((1, 0) if "lut" in forms else (1,)):
            for hbits in ((1, 0) if "hlut" in forms else (1,)):
                _check_generated_eval(tmp_path, src, prog, nrec, nprim, lut, hbits)


def test_lane_bvh_drops_terms_it_rejects(hostonly):
    """((a \\ b) \\ c) u d is a union of conjunctions, but one has three literals and the lanes'
    term records hold two: the builder takes the general form and carries no terms.  (It used
    to keep the terms it had just rejected, wrote their records past a two-literal buffer on
    its stack and told the launch to run term mode over them.)"""
    r = wl.Renderer("long", max_nodes=16)
    a, b, c, d = (r.sphere(rad) for rad in (1.0, 0.5, 0.4, 0.6))
    ab = r.difference(wl.arg(a), wl.arg(b, (0.7, 0.0, 0.0)))
    abc = r.difference(wl.arg(ab), wl.arg(c, (-0.7, 0.0, 0.0)))
    r.union(wl.arg(abc), wl.arg(d, (0.0, 1.5, 0.0)))
    prog, nrec, nprim = r.program()
    mats, nm = r.materials()
    desc = wl.lane_bvh(prog, nrec, nprim, mats, nm)[0]
    assert nprim == 4 and (desc.terms, desc.general, desc.wide) == (0, 1, 0)
    r.close()


def test_term_mode_ends_at_64_primitives(hostonly):
    """The exact pairs move across their boundaries with the size alone: 64 primitives are
    term mode, 65 are not; 32 fit one membership word, 33 take two."""
    got = {}
    for n in (32, 33, 64, 65):
        r = wl.Renderer("edge", max_nodes=1024)
        gs.build(r, "pairs", n, 1, exact=True)
        d = gs.describe(r)
        assert d["nprim"] == n
        got[n] = ("term" in d["forms"], d["words"])
        r.close()
    assert got == {32: (True, 1), 33: (True, 2), 64: (True, 2), 65: (False, 3)}


# ---- ray queries: the batch of a row, and a batch of hits against the float64 classifier -------

N_RAYS = 1000  # no multiple of 64
_BATCHES = {}


def ray_batch(r, case):
    """test_gpu_rays.make_batch for a row: about 1 000 seeded rays in its four groups, the box of
    group (b) what the row's camera sees.  The oracle's pass is made once per row and shared."""
    from test_gpu_rays import make_batch

    if case.name not in _BATCHES:
        look_from, look_at = (np.array(v, dtype=np.float64) for v in case.cam[:2])
        half = np.tan(np.radians(0.5 * case.cam[2])) * np.linalg.norm(look_from - look_at)
        sc, rays, exp = make_batch(r, case.name, n=N_RAYS, nb=400, step=6, box=(look_at - half, look_at + half),
                                   seed=2000 + case.seed)
        rays.setflags(write=False)
        exp.setflags(write=False)
        _BATCHES[case.name] = (sc, rays, exp)
    return _BATCHES[case.name]


def hits_vs_classifier(sh, rays, hits, what):
    """Every hit of a batch (Wo_RayHit rows: the oracle's, or a device's) against the float64
    classifier: membership differs across t -+ 2e-4 max(1, t) and RAY_ENTERS is the
    classifier's membership behind the hit; hits with another boundary that close are skipped
    as ambiguous, at most 20 % of them (test_scene_compile's cap)."""
    on = np.flatnonzero((hits["flags"] & wl.RAY_HIT) != 0)
    o, d = rays[on, 0:3].astype(np.float64), rays[on, 4:7].astype(np.float64)
    t = hits["t"][on].astype(np.float64)
    eps = 2e-4 * np.maximum(1.0, t)
    before = sh.scene_inside_many(o + (t - eps)[:, None] * d)
    after = sh.scene_inside_many(o + (t + eps)[:, None] * d)
    clear = before != after
    enters = (hits["flags"][on] & wl.RAY_ENTERS) != 0
    bad = on[clear & (after != enters)]
    print(what, "hits", len(on), "checked", int(clear.sum()))
    assert len(bad) == 0, (what, "RAY_ENTERS against the classifier at rays", bad[:8], hits[bad[:8]])
    assert clear.sum() >= 0.8 * len(on), (what, int(clear.sum()), len(on))


@pytest.mark.parametrize("name", NAMES)
def test_ray_batch_is_telling_and_the_oracle_matches_the_classifier(hostonly, name):
    """The batch the GPU file traces, judged on the oracle alone: enough hits and misses, and
    (rows without coincident surfaces) the oracle's own rows pass the classifier check the
    device's rows are put to, within its cap on ambiguous hits."""
    from test_gpu_rays import batch_is_telling

    case = BY_NAME[name]
    r, sh = make(case)
    _, rays, exp = ray_batch(r, case)
    telling = batch_is_telling(exp)
    print(name, telling)
    assert rays.shape == (N_RAYS, 8)
    assert telling["hit"] >= 0.15 and telling["miss"] >= 0.05, telling
    if not case.want.get("ties"):
        hits_vs_classifier(sh, rays, exp, name)
    r.close()
