"""The path tracer's shading pinned to a float64 Monte-Carlo reference (CPU only).

GPU frames are checked bit for bit against oracle/oracle.c, which states the shading of
DESIGN.md section 3.1 a second time in the same hand as the kernels.  Here the oracle itself
meets an independent statement (tests/shading_ref.py), in three steps:

  a. the reference equals closed forms where there are any (a Lambertian sphere, a mirror
     sphere, the Schlick series of a glass slab at six depth limits, a pool seen from inside
     past the critical angle);
  b. the oracle's frames of the physics scenes equal the reference's within 6 standard errors
     per pixel and per 4 x 4 block, the variance being the reference's own;
  c. each of thirteen deliberate errors, switched on in the reference, is seen by the same
     comparison at 12 standard errors or more -- so b has the power to notice them.

All seeds are fixed: every test is one draw.
"""
import numpy as np
import pytest

import physics_scenes as ps
import pyoracle
import shading_ref as sr
from csgrenderer_amd import wololo as wl

Z_ACCEPT = 6.0   # two-sided normal tail 2e-9; fewer than 1e5 cells in this file
Z_CAUGHT = 12.0  # twice the acceptance bound
SPP = {case: 4096 for case in ps.CASES}  # samples per pixel, oracle and reference alike
SPP["glass_slab", 4] = 16384
SPP["defocus", 8] = 16384
REF_SEED, ORACLE_SEED = 20, 5

_cache = {}


def reference(name, depth, mutate=None):
    key = ("ref", name, depth, mutate)
    if key not in _cache:
        rec = ps.make(name)
        _cache[key] = sr.render(rec, ps.W, ps.H, SPP[name, depth], depth, seed=REF_SEED, mutate=mutate)
        rec.close()
    return _cache[key]


def oracle(name, depth):
    key = ("oracle", name, depth)
    if key not in _cache:
        rec = ps.make(name)
        prog, nrec, _ = rec.r.program()
        mats, nm = rec.r.materials()
        p = wl.render_params(ps.W, ps.H, spp=SPP[name, depth], max_depth=depth, seed=ORACLE_SEED, mode=wl.MODE_PATHTRACE)
        img, _ = pyoracle.pathtrace_rows(prog, nrec, mats, nm, rec.r.frame_desc(p), 0, ps.H)
        rec.close()
        _cache[key] = img[..., :3].astype(np.float64)
    return _cache[key]


def oracle_z(name, depth, mutate=None, own_variance=True):
    """z of every pixel cell and of every 4 x 4 block cell, oracle against reference.  The
    variance is the compared reference's own, or (own_variance=False) the unmutated one's."""
    img = oracle(name, depth)
    mean, var, n = reference(name, depth, mutate)
    if not own_variance:
        var = reference(name, depth)[1]
    inv_n = 1.0 / SPP[name, depth] + 1.0 / n
    zp = ps.z_scores(img, mean, var, inv_n)
    bm, bv = ps.block_cells(mean, var)
    zb = ps.z_scores(ps.block_cells(img, var)[0], bm, bv, inv_n)
    return zp, zb


def test_flattened_scene_classifies_like_the_recorded_graph(hostonly):
    """shading_ref.Scene composes the placements once; the recorded-graph classifier walks them
    per point.  Same membership on random points of csg32 (rotations: test_marshalling's cluster)."""
    from test_marshalling import _big_union_cluster
    for rec, lo, hi in ((ps.make("csg32_small"), (-7, -1, -7), (7, 3.5, 7)), (_big_union_cluster(), (-6, -6, -6), (6, 6, 6))):
        P = np.random.default_rng(1).uniform(lo, hi, (20000, 3))
        want, dist = rec.scene_classify(P)
        got = sr.Scene(rec).inside(P)
        assert 0.02 * len(P) < want.sum() < 0.98 * len(P)
        assert (got == want)[dist > 1e-9].all()
        rec.close()


# ---- a. the reference against mathematics ------------------------------------------------------
CLOSED_CASES = [(n, d) for n, d in ps.CASES if n in ps.CLOSED_FORM]


@pytest.mark.parametrize("name,depth", CLOSED_CASES)
def test_reference_matches_the_closed_form(hostonly, name, depth):
    want, var, valid, cls = ps.closed_form(name, depth)
    q = ps.quadrature_error(name, depth)
    share = valid.mean()
    print(f"{name} depth {depth}: q = {q:.3g}, share of cells {share:.3f}")
    assert share >= 0.6, share
    assert q < 1e-3, q  # the quadrature is not what the bound rests on
    mean, _, n = reference(name, depth)
    z = ps.z_scores(mean, want, var, 1.0 / n, q=q, exact=1e-12)[valid]
    print(f"  largest z {z.max():.2f} over {z.size} cells")
    assert z.max() <= Z_ACCEPT, (name, depth, float(z.max()))
    bm, bv = ps.block_cells(np.where(valid[..., None], want, 0.0), np.where(valid[..., None], var, 0.0))
    zb = ps.z_scores(ps.block_cells(np.where(valid[..., None], mean, 0.0), var)[0], bm, bv, 1.0 / n, q=q, exact=1e-12)
    print(f"  largest block z {zb.max():.2f}")
    assert zb.max() <= Z_ACCEPT, (name, depth, float(zb.max()))
    if name == "tir_pool":
        # beyond the critical angle the closed form is sky(reflected) alone, no Schlick draw: a cell's
        # only spread is its footprint's, and such cells are a good part of the frame
        tir = valid & cls
        assert 0.2 < tir.mean() < 0.8, tir.mean()
        assert var[tir].max() < 1e-4 < var[valid & ~cls].max()


# ---- b. the oracle against the reference -------------------------------------------------------
@pytest.mark.parametrize("name,depth", ps.CASES)
def test_oracle_matches_the_reference(hostonly, name, depth):
    zp, zb = oracle_z(name, depth)
    print(f"{name} depth {depth}: largest z {zp.max():.2f} per pixel, {zb.max():.2f} per block")
    assert zp.max() <= Z_ACCEPT, (name, depth, float(zp.max()), np.argwhere(zp > Z_ACCEPT)[:5])
    assert zb.max() <= Z_ACCEPT, (name, depth, float(zb.max()), np.argwhere(zb > Z_ACCEPT)[:5])


# ---- c. power: every mutant of the reference is caught ------------------------------------------
CAUGHT_BY = {
    "lambert_uniform": ("lambert_sphere", 2),
    "fuzz_ball": ("fuzzy_sphere_10", 2),
    "metal_no_absorb": ("fuzzy_sphere_10", 8),
    "schlick_pow4": ("glass_slab", 2),
    "schlick_cos_transmitted": ("glass_slab", 8),
    "ior_swapped": ("glass_sphere", 8),
    "no_tir": ("tir_pool", 8),
    "lens_r_linear": ("defocus", 8),
    "no_jitter": ("mirror_sphere", 2),
    "row_flip": ("lambert_sphere", 2),
    "sky_unnormalised": ("lambert_sphere", 2),
    "depth_plus_one": ("glass_slab", 3),
    "limit_returns_sky": ("glass_slab", 1),
}


def test_every_mutant_has_a_catching_scene():
    assert sorted(CAUGHT_BY) == sorted(sr.MUTANTS) and len(sr.MUTANTS) == 13


@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_mutant_is_caught(hostonly, mutant):
    """Twice over: with the mutated reference's own variance (the comparison as it would run were
    the reference wrong in this way), and with the unmutated reference's, the standard error of
    step b's own bound.  The second is finite wherever the scene has any spread: a mutant can
    make a cell deterministic (no_jitter), and then the first says only "beyond 2^-20"."""
    name, depth = CAUGHT_BY[mutant]
    zp, zb = oracle_z(name, depth, mutant)
    z = max(float(zp.max()), float(zb.max()))
    fp, fb = oracle_z(name, depth, mutant, own_variance=False)
    f = max(float(fp.max()), float(fb.max()))
    gap = float(np.abs(oracle(name, depth) - reference(name, depth, mutant)[0]).max())
    print(f"{mutant}: {name} depth {depth}: own variance z = {zp.max():.1f} per pixel, {zb.max():.1f} per block; "
          f"unmutated variance z = {fp.max():.1f}, {fb.max():.1f}; largest |difference| {gap:.3f}")
    assert z >= Z_CAUGHT, (mutant, name, depth, z)
    assert f >= Z_CAUGHT, (mutant, name, depth, f)
