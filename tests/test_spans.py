"""Ray span queries and point classification, the host side (CPU only): the ABI of Wo_RaySpans /
Wo_RayCrossing, the loud failure without a device, and the references the GPU tests compare
against -- pinned here to the oracle's first-hit query, to the float64 classifier of the
recorded node graph, and judged for how telling their batches are."""
import ctypes

import numpy as np
import pytest

import span_support as sp
import test_gpu_rays as tgr
from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl
from recorder import Recorder

MAX_REF = 64  # more crossings than any ray of these batches has


@pytest.fixture(scope="module")
def span_lib(tmp_path_factory):
    return sp.build_span_ref(tmp_path_factory.mktemp("span_ref"))


def _recorded(scene):
    rec = Recorder(scene)
    scenes.build(scene, rec)
    return rec


@pytest.mark.parametrize("cname,mirror,fields", [("Wo_RayCrossing", wl.RayCrossing, wl.RAY_CROSSING_FIELDS),
                                                 ("Wo_RaySpans", wl.RaySpans, wl.RAY_SPANS_FIELDS)])
def test_span_abi_layout(cname, mirror, fields):
    assert ctypes.sizeof(mirror) == 16 and wl.abi_layout(cname) == 16
    dt = np.dtype(fields)
    assert dt.itemsize == 16 and [f[0] for f in fields] == [f[0] for f in mirror._fields_]
    for fname, _ in mirror._fields_:
        assert wl.abi_layout(cname, fname) == getattr(mirror, fname).offset == dt.fields[fname][1], (cname, fname)
    assert (wl.RAY_INSIDE, wl.RAY_TRUNCATED, wl.POINT_INSIDE, wl.POINT_INVALID) == (16, 32, 1, 8)


def test_spans_and_points_without_device_fail_loudly(hostonly):
    r = wl.Renderer("nodev", max_nodes=4)
    r.sphere(1.0)
    rays = np.zeros((3, 8), dtype=np.float32)
    rays[:, 6] = -1.0
    pts = np.zeros((3, 4), dtype=np.float32)
    calls = (lambda: r.trace_spans(rays, 4), lambda: r.trace_spans(rays, 0),
             lambda: r.trace_spans_device(0x1000, 0x2000, 0x3000, 3, 4), lambda: r.classify_points(pts),
             lambda: r.classify_points_device(0x1000, 0x2000, 3))
    for call in calls:
        wl.clear_error()
        with pytest.raises(wl.WololoError, match="device"):
            call()
    buf = rays.ctypes.data
    assert r.lib.wo_renderer_trace_spans(r.ptr, buf, buf, buf, 3, 1) == -1
    assert r.lib.wo_renderer_trace_spans_device(r.ptr, buf, buf, None, 3, 0, None) == -1
    assert r.lib.wo_renderer_classify_points(r.ptr, buf, buf, 3) == -1
    assert r.lib.wo_renderer_classify_points_device(r.ptr, buf, buf, 3, None) == -1
    assert r.ray_path() == "none"
    r.close()


@pytest.mark.parametrize("scene", ["csg32", "csg32_union", "csg32_nested", "rtiow_cover"])
def test_reference_crossing_0_is_the_oracles_hit(hostonly, span_lib, scene):
    """The reference's first crossing on make_batch's rays is pyoracle.trace's hit, field by field;
    it reports no crossing exactly where the oracle misses.  Also: these rays start inside often
    enough, and csg32_union's coincident planes give crossings of equal t."""
    r = wl.Renderer(scene, max_nodes=4096)
    scenes.build(scene, r)
    _, rays, exp = tgr.make_batch(r, scene)
    spans, cross = sp.SpanScene(span_lib, r).expect(rays, MAX_REF)
    assert (spans["flags"] & (wl.RAY_INVALID | wl.RAY_TRUNCATED)).max() == 0
    hit = (exp["flags"] & wl.RAY_HIT) != 0
    assert ((spans["count"] == 0) == ~hit).all()
    for name in ("t", "flags", "leaf", "node"):
        assert cross[name][0, hit].tobytes() == np.ascontiguousarray(exp[name][hit]).tobytes(), (scene, name)
    inside = ((spans["flags"] & wl.RAY_INSIDE) != 0).mean()
    print(scene, "start inside", inside)
    assert inside >= 0.05, (scene, inside)
    if scene == "csg32_union":
        assert _equal_t_pairs(spans, cross) >= 1
    r.close()


def _equal_t_pairs(spans, cross):
    k = np.arange(cross.shape[0] - 1)[:, None]
    both = k + 1 < spans["stored"][None, :]
    return int((both & (cross["t"][:-1] == cross["t"][1:])).sum())


@pytest.mark.parametrize("scene", ["csg32", "csg32_nested", "csg256_chain", "rtiow_cover"])
def test_reference_spans_match_the_node_graph(hostonly, span_lib, scene):
    """Between consecutive boundaries (from WO_T_MIN; the last segment taken 1.0 long) the float64
    classifier of the recorded graph says inside / outside as the spans alternate from
    WO_RAY_INSIDE.  A segment is judged when it is longer than 2 eps, eps = 2e-4 max(1, t), and
    its midpoint is more than 2e-4 from any surface (test_marshalling's band)."""
    rec = _recorded(scene)
    rays = sp.through_rays(scene)
    ref = sp.SpanScene(span_lib, rec.r).reference(rays, MAX_REF)
    assert ref["count"].max() <= MAX_REF
    o = rays[:, 0:3].astype(np.float64)
    d = rays[:, 4:7].astype(np.float64)
    pts, want, long_enough = [], [], []
    for i in range(len(rays)):
        c = int(ref["count"][i])
        bounds = np.concatenate([[wl.WO_T_MIN], ref["t"][i, :c].astype(np.float64)])
        bounds = np.append(bounds, bounds[-1] + 1.0)
        mid = 0.5 * (bounds[:-1] + bounds[1:])
        eps = 2e-4 * np.maximum(1.0, bounds[1:])
        pts.append(o[i] + mid[:, None] * d[i])
        want.append((np.arange(c + 1) + int(ref["inside0"][i])) % 2 == 1)
        long_enough.append(bounds[1:] - bounds[:-1] > 2 * eps)
    pts, want, long_enough = np.concatenate(pts), np.concatenate(want), np.concatenate(long_enough)
    got, dist = rec.scene_classify(pts)
    judged = long_enough & (dist > 2e-4)
    share = judged.mean()
    print(scene, "segments", len(pts), "judged", share, "disagree", int((judged & (got != want)).sum()))
    assert share >= 0.99, (scene, share)
    assert not (judged & (got != want)).any(), (scene, pts[judged & (got != want)][:3])
    rec.close()


@pytest.mark.parametrize("scene", sp.POINT_SCENES)
def test_point_reference_matches_the_node_graph(hostonly, scene):
    rec = _recorded(scene)
    prog, nrec, _ = rec.r.program()
    P = sp.sample_points(rec, scene)
    got = sp.classify_points_f32(prog, nrec, P)
    want, dist = rec.scene_classify(P.astype(np.float64))
    band = dist <= 2e-4
    print(scene, "points", len(P), "inside", want.mean(), "in band", band.mean(), "in-band disagreements",
          int((band & (got != want)).sum()))
    assert not ((got != want) & ~band).any(), (scene, P[(got != want) & ~band][:3])
    assert band.mean() <= 0.03, (scene, band.mean())
    assert 0.02 < want.mean() < 0.98, (scene, want.mean())
    rec.close()


def _through_stats(span_lib, scene):
    r = wl.Renderer(scene, max_nodes=4096)
    scenes.build(scene, r)
    sc = sp.SpanScene(span_lib, r)
    rays = sp.through_rays(scene)
    ref = sc.reference(rays, MAX_REF)
    spans, cross = sc.expect(rays, MAX_REF)
    r.close()
    return ref, spans, cross


def test_through_rays_are_telling(hostonly, span_lib):
    """Judged on the reference alone, so a weak batch fails here and not silently on the GPU: many
    crossings and many events per ray (windows of 4, 8 and 16 keys all overflow), and ties."""
    ref, _, _ = _through_stats(span_lib, "csg256_chain")
    shares = {"chain >4 crossings": (ref["count"] > 4).mean(), "chain >16 events": (ref["events"] > 16).mean()}
    assert shares["chain >4 crossings"] >= 0.40 and shares["chain >16 events"] >= 0.10, shares
    ref, _, _ = _through_stats(span_lib, "csg32_nested")
    shares["nested >8 events"] = (ref["events"] > 8).mean()
    assert shares["nested >8 events"] >= 0.35, shares
    ref, _, _ = _through_stats(span_lib, "rtiow_cover")
    shares["cover >16 crossings"] = (ref["count"] > 16).mean()
    shares["cover most crossings"] = int(ref["count"].max())
    assert shares["cover >16 crossings"] >= 0.01 and ref["count"].max() <= MAX_REF, shares
    _, spans, cross = _through_stats(span_lib, "csg32_union")
    shares["union equal-t pairs"] = _equal_t_pairs(spans, cross)
    print(shares)
