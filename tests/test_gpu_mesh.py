"""GPU: the surface mesh of the solid (wo_renderer_mesh*), bit for bit and row for row against the
numpy restatement of tests/mesh_support.py: counts, vertices, quads and ids on the four scenes at
both grids (partial waves in every pass), the two-cell minimum, no bisection, two workgroups, the
host form, the counts-only call, truncation, the buffers' limits, a scene edit, the refusals."""
import ctypes

import numpy as np
import pytest

import mesh_support as ms
import span_support as sp
from csgrenderer_amd import wololo as wl

pytestmark = pytest.mark.gpu

I32_SENTINEL = ms.SENTINEL - (1 << 32)
PAD = 3  # sentinel rows behind the rows a call may write
CASES = [(s, n, it) for s in ms.SCENES for n, it in ms.GRIDS]


def _grid(scene, n, iters):
    return ms.grid_of(*sp.BOXES[scene], n, iters)


class Buffers:
    """Sentinel-filled device buffers for one call: `rows_v` vertex rows, `rows_q` quad and id rows,
    the scratch with 64 sentinel bytes behind the stated size."""

    def __init__(self, grid, rows_v, rows_q, ids=True):
        import torch
        self.need = wl.mesh_scratch_bytes(grid)
        self.v = torch.full((max(rows_v, 1), 4), I32_SENTINEL, dtype=torch.int32, device="cuda")
        self.q = torch.full((max(rows_q, 1), 4), I32_SENTINEL, dtype=torch.int32, device="cuda")
        self.i = torch.full((max(rows_q, 1), 4), I32_SENTINEL, dtype=torch.int32, device="cuda") if ids else None
        self.c = torch.full((4,), I32_SENTINEL, dtype=torch.int32, device="cuda")
        self.s = torch.full((self.need // 4 + 16,), I32_SENTINEL, dtype=torch.int32, device="cuda")
        self.rows_v, self.rows_q = rows_v, rows_q

    def run(self, r, grid, max_v, max_q, counts_only=False):
        import torch
        if counts_only:
            r.mesh_device(grid, 0, 0, 0, 0, 0, self.c.data_ptr(), self.s.data_ptr(), self.need,
                          torch.cuda.current_stream().cuda_stream)
        else:
            r.mesh_device(grid, self.v.data_ptr(), max_v, self.q.data_ptr(), self.i.data_ptr() if self.i is not None else 0,
                          max_q, self.c.data_ptr(), self.s.data_ptr(), self.need, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return self

    def counts(self):
        return tuple(int(x) for x in self.c.cpu().numpy().view(np.uint32))

    def vertices(self):
        return self.v.cpu().numpy().view(np.uint32)[:self.rows_v]

    def quads(self):
        return self.q.cpu().numpy().view(np.uint32)[:self.rows_q]

    def ids(self):
        return self.i.cpu().numpy().view(np.uint32)[:self.rows_q]

    def scratch_tail(self):
        return self.s.cpu().numpy().view(np.uint32)[self.need // 4:]


def _words(a):
    """A structured or plain array as (rows, 4) uint32."""
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, f"{what}: {len(bad)} rows differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


def _check_full(buf, ref, what, ids=True):
    """A call whose maxima are the buffers' rows less PAD: every row of the reference, bit for bit, the
    sentinel in every row behind them and behind the scratch, the full counts and no truncation."""
    nv, nq, caps = ref["counts"]
    assert buf.counts() == (nv, nq, caps, 0), (what, buf.counts(), ref["counts"])
    v, q = buf.vertices(), buf.quads()
    _same(v[:nv], _words(ref["vertices"]), what + " vertices")
    _same(q[:nq], _words(ref["quads"]), what + " quads")
    assert (v[nv:] == ms.SENTINEL).all() and (q[nq:] == ms.SENTINEL).all(), what + ": a row beyond the counts was written"
    if ids:
        i = buf.ids()
        _same(i[:nq], _words(ref["ids"]), what + " ids")
        assert (i[nq:] == ms.SENTINEL).all(), what + ": an id row beyond the counts was written"
    assert (buf.scratch_tail() == ms.SENTINEL).all(), what + ": the scratch was written past wo_mesh_scratch_bytes"


def _full(r, grid, ref, ids=True):
    nv, nq, _ = ref["counts"]
    return Buffers(grid, nv + PAD, nq + PAD, ids).run(r, grid, nv + PAD, nq + PAD)


@pytest.mark.parametrize("scene,n,iters", CASES, ids=[f"{s}-{n[0]}x{n[1]}x{n[2]}" for s, n, _ in CASES])
def test_parity_with_the_reference(scene, n, iters):
    """68 * 22 * 46 and 14 * 8 * 12 corners are no multiples of 64, nor are the counts: every pass
    has a partial wave.  The maxima exceed the counts, so the rows behind them must stay."""
    ref = ms.scene_reference(scene, n, iters)
    r = ms.scene_renderer(scene)
    grid = _grid(scene, n, iters)
    _check_full(_full(r, grid, ref), ref, f"{scene} {n}")
    r.close()


def _sphere(radius):
    r = wl.Renderer("sphere", max_nodes=8)
    r.sphere(radius)
    return r


def _reference_of(r, lo, hi, n, iters):
    prog, nrec, _ = r.program()
    return ms.reference_mesh(prog, nrec, r.program_nodes(), r.materials()[1], lo, hi, n, iters)


def test_the_two_cell_minimum():
    """n = (2, 2, 2) round one small sphere: one interior corner, six quads, eight vertices."""
    r = _sphere(0.3)
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    ref = _reference_of(r, lo, hi, (2, 2, 2), 16)
    assert ref["counts"] == (8, 6, 0)
    grid = ms.grid_of(lo, hi, (2, 2, 2), 16)
    _check_full(_full(r, grid, ref), ref, "two cells")
    r.close()


def test_empty_scene():
    """No node at all: zero counts, no row written, and the host form returns no arrays."""
    r = wl.Renderer("empty", max_nodes=4)
    lo, hi, n = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (4, 5, 6)
    ref = _reference_of(r, lo, hi, n, 8)
    assert ref["counts"] == (0, 0, 0)
    grid = ms.grid_of(lo, hi, n, 8)
    _check_full(_full(r, grid, ref), ref, "empty scene")
    vertices, quads, ids, counts = r.mesh(grid)
    assert len(vertices) == 0 and quads.shape == (0, 4) and len(ids) == 0 and counts.quads == 0 and counts.flags == 0
    r.close()


def test_no_bisection():
    scene, n = "csg256_chain", (13, 7, 11)
    ref = ms.scene_reference(scene, n, 0)
    assert ref["counts"][1] >= 100 and ref["counts"][2] > 0
    r = ms.scene_renderer(scene)
    grid = _grid(scene, n, 0)
    _check_full(_full(r, grid, ref), ref, "iters 0")
    r.close()


@pytest.mark.parametrize("scene", ms.SCENES)
def test_two_workgroups(scene, monkeypatch):
    """The same rows whatever the launch geometry: WOLOLO_RAY_BLOCKS=2 bounds every pass's grid."""
    monkeypatch.setenv("WOLOLO_RAY_BLOCKS", "2")
    r = ms.scene_renderer(scene)
    for n, iters in ms.GRIDS if scene == "csg256_chain" else ms.GRIDS[:1]:
        ref = ms.scene_reference(scene, n, iters)
        grid = _grid(scene, n, iters)
        _check_full(_full(r, grid, ref), ref, f"{scene} {n} two workgroups")
    r.close()


def test_host_form_equals_the_device_form():
    scene, (n, iters) = "csg256_chain", ms.GRIDS[1]
    ref = ms.scene_reference(scene, n, iters)
    r = ms.scene_renderer(scene)
    grid = _grid(scene, n, iters)
    vertices, quads, ids, counts = r.mesh(grid)
    assert (counts.vertices, counts.quads, counts.cap_quads, counts.flags) == (*ref["counts"], 0)
    _same(_words(vertices), _words(ref["vertices"]), "host form vertices")
    _same(_words(quads), _words(ref["quads"]), "host form quads")
    _same(_words(ids), _words(ref["ids"]), "host form ids")
    # the C call itself: arrays for a mesh with rows, NULLs and zero counts after wo_mesh_free
    m = wl.Mesh()
    assert r.lib.wo_renderer_mesh(r.ptr, ctypes.byref(grid), ctypes.byref(m)) == 0
    assert m.vertices and m.quads and m.quad_ids and m.counts.quads == ref["counts"][1]
    assert ctypes.string_at(m.quads, 16 * m.counts.quads) == ref["quads"].tobytes()
    r.lib.wo_mesh_free(ctypes.byref(m))
    assert not m.vertices and not m.quads and not m.quad_ids
    assert (m.counts.vertices, m.counts.quads, m.counts.cap_quads, m.counts.flags) == (0, 0, 0, 0)
    r.close()


def test_counts_only_call():
    scene, (n, iters) = "rtiow_cover", ms.GRIDS[0]
    ref = ms.scene_reference(scene, n, iters)
    r = ms.scene_renderer(scene)
    grid = _grid(scene, n, iters)
    buf = Buffers(grid, PAD, PAD).run(r, grid, 0, 0, counts_only=True)
    assert buf.counts()[:3] == ref["counts"]
    assert buf.counts()[3] == wl.MESH_TRUNCATED  # the counts exceed maxima of 0
    assert (buf.vertices() == ms.SENTINEL).all() and (buf.quads() == ms.SENTINEL).all() and (buf.ids() == ms.SENTINEL).all()
    assert (buf.scratch_tail() == ms.SENTINEL).all()
    r.close()


def test_truncation():
    scene, (n, iters) = "csg256_chain", ms.GRIDS[1]
    ref = ms.scene_reference(scene, n, iters)
    nv, nq, caps = ref["counts"]
    r = ms.scene_renderer(scene)
    grid = _grid(scene, n, iters)
    hv, hq = nv // 2, nq // 2
    for with_ids in (True, False):
        buf = Buffers(grid, nv, nq, with_ids).run(r, grid, hv, hq)
        assert buf.counts() == (nv, nq, caps, wl.MESH_TRUNCATED)
        v, q = buf.vertices(), buf.quads()
        _same(v[:hv], _words(ref["vertices"])[:hv], "truncated vertices")
        _same(q[:hq], _words(ref["quads"])[:hq], "truncated quads")  # the indices keep the full numbering
        assert (q[:hq] >= hv).any()
        assert (v[hv:] == ms.SENTINEL).all() and (q[hq:] == ms.SENTINEL).all(), "a row at or beyond the maximum was written"
        if with_ids:
            i = buf.ids()
            _same(i[:hq], _words(ref["ids"])[:hq], "truncated ids")
            assert (i[hq:] == ms.SENTINEL).all()
    # one maximum alone exceeded; vertices alone (max_quads 0 with a NULL quad buffer)
    buf = Buffers(grid, nv, nq).run(r, grid, nv, hq)
    assert buf.counts() == (nv, nq, caps, wl.MESH_TRUNCATED)
    _same(buf.vertices(), _words(ref["vertices"]), "all vertices")
    import torch
    only = Buffers(grid, nv + PAD, PAD)
    r.mesh_device(grid, only.v.data_ptr(), nv + PAD, 0, 0, 0, only.c.data_ptr(), only.s.data_ptr(), only.need,
                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert only.counts() == (nv, nq, caps, wl.MESH_TRUNCATED)
    _same(only.vertices()[:nv], _words(ref["vertices"]), "vertices alone")
    assert (only.vertices()[nv:] == ms.SENTINEL).all()
    r.close()


def test_scene_edit():
    """Mesh, add a sphere that sticks out of the solid, mesh again: the new scene's mesh."""
    lo, hi, n, iters = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), (9, 10, 11), 8
    r = wl.Renderer("edit", max_nodes=16)
    a = r.sphere(1.0)
    grid = ms.grid_of(lo, hi, n, iters)
    before = _reference_of(r, lo, hi, n, iters)
    _check_full(_full(r, grid, before), before, "before the edit")
    r.union(wl.arg(a), wl.arg(r.sphere(0.7), (0.9, 0.2, -0.3)))
    after = _reference_of(r, lo, hi, n, iters)
    assert after["counts"] != before["counts"]
    _check_full(_full(r, grid, after), after, "after the edit")
    r.close()


def _refused(text, call, *args):
    wl.clear_error()
    with pytest.raises(wl.WololoError, match=text):
        call(*args)


def test_refusals():
    """Every refusal stops at the argument checks: nothing is launched, no buffer is touched."""
    import torch
    scene, (n, iters) = "csg32", ms.GRIDS[0]
    r = ms.scene_renderer(scene)
    grid = _grid(scene, n, iters)
    b = Buffers(grid, 8, 8)
    v, q, i, c, s = (t.data_ptr() for t in (b.v, b.q, b.i, b.c, b.s))
    _refused("16-byte aligned", r.mesh_device, grid, v + 4, 8, q, i, 8, c, s, b.need)
    _refused("16-byte aligned", r.mesh_device, grid, v, 8, q + 8, i, 8, c, s, b.need)
    _refused("16-byte aligned", r.mesh_device, grid, v, 8, q, i + 4, 8, c, s, b.need)
    _refused("16-byte aligned", r.mesh_device, grid, v, 8, q, i, 8, c + 4, s, b.need)
    _refused("16-byte aligned", r.mesh_device, grid, v, 8, q, i, 8, c, s + 8, b.need)
    _refused("NULL counts", r.mesh_device, grid, v, 8, q, i, 8, 0, s, b.need)
    _refused("NULL scratch", r.mesh_device, grid, v, 8, q, i, 8, c, 0, b.need)
    _refused("NULL vertex", r.mesh_device, grid, 0, 8, q, i, 8, c, s, b.need)
    _refused("NULL quad", r.mesh_device, grid, v, 8, 0, i, 8, c, s, b.need)
    _refused("short of", r.mesh_device, grid, v, 8, q, i, 8, c, s, b.need - 1)
    bad = _grid(scene, n, iters)
    bad.iters = 25
    _refused("bisection steps", r.mesh_device, bad, v, 8, q, i, 8, c, s, b.need)
    _refused("bisection steps", r.mesh, bad)
    _refused("NULL grid", r.mesh_device, None, v, 8, q, i, 8, c, s, b.need)
    assert r.lib.wo_renderer_mesh(r.ptr, ctypes.byref(grid), None) == -1 and "NULL result" in wl.last_error()
    torch.cuda.synchronize()
    for t in (b.v, b.q, b.i, b.c, b.s):
        assert (t.cpu().numpy().view(np.uint32) == ms.SENTINEL).all()
    r.close()


def test_other_state_is_left_alone():
    """ray_path() is what it was (as after point classification), and the caller's other results --
    ray hits and point classes made before -- are what the same calls give afterwards."""
    scene, (n, iters) = "csg32", ms.GRIDS[0]
    ref = ms.scene_reference(scene, n, iters)
    r = ms.scene_renderer(scene)
    grid = _grid(scene, n, iters)
    assert r.ray_path() == "none"
    _check_full(_full(r, grid, ref), ref, "before any ray launch")
    assert r.ray_path() == "none"
    rays = sp.through_rays(scene, n=256)
    hits = r.trace_rays(rays)
    path = r.ray_path()
    pts = np.random.default_rng(3).uniform(-3, 3, size=(500, 3)).astype(np.float32)
    classes = r.classify_points(pts)
    vertices, quads, ids, _ = r.mesh(grid)
    _check_full(_full(r, grid, ref), ref, "after a ray launch")
    assert r.ray_path() == path
    assert r.trace_rays(rays).tobytes() == hits.tobytes()
    assert (r.classify_points(pts) == classes).all()
    assert vertices.tobytes() == ref["vertices"].tobytes() and quads.tobytes() == ref["quads"].tobytes()
    r.close()
