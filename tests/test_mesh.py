"""The surface mesh of the solid, the host side (CPU only): the ABI of the mesh's structs,
wo_mesh_grid_check and wo_mesh_scratch_bytes on a table, the loud failure without a device, the
numpy reference the GPU tests compare against (tests/mesh_support.py) pinned to things it shares no
code with (closedness, orientation, a sphere's radius, the clip box's faces, the leaf tests), the
OBJ writer's round trip, and csrc/mesh.c's stand-alone driver under ASan + UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mesh_support as ms
import span_support as sp
from csgrenderer_amd import wololo as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csgrenderer_amd", "csrc")
CASES = [(s, n, it) for s in ms.SCENES for n, it in ms.GRIDS]
CASE_IDS = [f"{s}-{n[0]}x{n[1]}x{n[2]}" for s, n, _ in CASES]


# field offsets as the issue's declarations lay them out
LAYOUTS = {
    "Wo_MeshGrid": (wl.MeshGrid, 48, {"lo": 0, "hi": 12, "n": 24, "iters": 36, "flags": 40, "reserved": 44}),
    "Wo_MeshVertex": (wl.MeshVertex, 16, {"p": 0, "cell": 12}),
    "Wo_MeshQuad": (wl.MeshQuad, 16, {"v": 0}),
    "Wo_MeshQuadIds": (wl.MeshQuadIds, 16, {"leaf": 0, "node": 4, "material": 8, "flags": 12}),
    "Wo_MeshCounts": (wl.MeshCounts, 16, {"vertices": 0, "quads": 4, "cap_quads": 8, "flags": 12}),
}


@pytest.mark.parametrize("cname", sorted(LAYOUTS))
def test_mesh_abi_layout(cname):
    mirror, size, offsets = LAYOUTS[cname]
    assert ctypes.sizeof(mirror) == size == wl.abi_layout(cname)
    assert [f for f, _ in mirror._fields_] == list(offsets)
    for fname, off in offsets.items():
        assert wl.abi_layout(cname, fname) == getattr(mirror, fname).offset == off, (cname, fname)
    assert wl.abi_layout("Wo_Mesh") == ctypes.sizeof(wl.Mesh)
    for fname, _ in wl.Mesh._fields_:
        assert wl.abi_layout("Wo_Mesh", fname) == getattr(wl.Mesh, fname).offset
    assert np.dtype(wl.MESH_VERTEX_FIELDS).itemsize == 16 and np.dtype(wl.MESH_QUAD_IDS_FIELDS).itemsize == 16
    assert (wl.MESH_MAX_CELLS, wl.MESH_TRUNCATED, wl.MESH_QUAD_AXIS, wl.MESH_QUAD_POSITIVE, wl.MESH_QUAD_CAP) == (1024, 1, 3, 4, 8)


# ---- the grid check ----
GOOD = dict(lo=(-1, -1, -1), hi=(1, 1, 1), n=(4, 4, 4), iters=8, flags=0, reserved=0)
# in the stated order of the checks; a case that fails several names the first
BAD_GRIDS = [
    ("nan", dict(lo=(np.nan, -1, -1)), "not finite"),
    ("inf", dict(hi=(1, np.inf, 1)), "not finite"),
    ("nan before lo >= hi", dict(lo=(-1, 5, -1), hi=(1, 1, np.nan)), "not finite"),
    ("lo == hi", dict(lo=(-1, 1, -1)), "lo < hi"),
    ("lo > hi", dict(hi=(1, 1, -2)), "lo < hi"),
    ("lo >= hi before the counts", dict(hi=(1, 1, -2), n=(0, 4, 4)), "lo < hi"),
    ("one cell", dict(n=(4, 1, 4)), "cells on axis 1"),
    ("no cell", dict(n=(0, 4, 4)), "cells on axis 0"),
    ("1025 cells", dict(n=(4, 4, 1025)), "cells on axis 2"),
    ("counts before iters", dict(n=(4, 4, 1025), iters=25), "cells on axis 2"),
    ("iters 25", dict(iters=25), "bisection steps"),
    ("iters before flags", dict(iters=25, flags=1), "bisection steps"),
    ("flags", dict(flags=2), "flags must be 0"),
    ("flags before reserved", dict(flags=1, reserved=1), "flags must be 0"),
    ("reserved", dict(reserved=1), "reserved must be 0"),
    ("reserved before h", dict(reserved=1, lo=(-3e38, -1, -1), hi=(3e38, 1, 1)), "reserved must be 0"),
    ("extent overflows", dict(lo=(-3e38, -1, -1), hi=(3e38, 1, 1)), "cell size on axis 0"),
    ("h underflows", dict(lo=(-1, -1, 0), hi=(1, 1, 1e-45), n=(4, 4, 4)), "cell size on axis 2"),
]


def _grid(**over):
    kw = dict(GOOD)
    kw.update(over)
    return ms.grid_of(kw["lo"], kw["hi"], kw["n"], kw["iters"], kw["flags"], kw["reserved"])


@pytest.mark.parametrize("name,over,text", BAD_GRIDS, ids=[b[0] for b in BAD_GRIDS])
def test_bad_grid_is_refused(name, over, text):
    g = _grid(**over)
    lib = wl.load()
    h = (ctypes.c_float * 3)(7.0, 7.0, 7.0)
    wl.clear_error()
    assert lib.wo_mesh_grid_check(ctypes.byref(g), h) == -1
    assert "mesh grid" in wl.last_error() and text in wl.last_error(), wl.last_error()
    assert list(h) == [7.0, 7.0, 7.0]
    wl.clear_error()
    assert lib.wo_mesh_scratch_bytes(ctypes.byref(g)) == 0 and text in wl.last_error()
    with pytest.raises(wl.WololoError, match="mesh grid"):
        wl.mesh_grid_check(g)
    with pytest.raises(wl.WololoError, match="mesh grid"):
        wl.mesh_scratch_bytes(g)


def test_null_grid_is_refused():
    lib = wl.load()
    wl.clear_error()
    assert lib.wo_mesh_grid_check(None, None) == -1 and "NULL grid" in wl.last_error()
    assert lib.wo_mesh_scratch_bytes(None) == 0


def test_cell_sizes_match_the_numpy_expression():
    rng = np.random.default_rng(11)
    cases = [((-2, -2, -2), (2, 2, 2), (32, 32, 32)), ((0, 0, 0), (1, 1, 1), (2, 3, 1024)),
             ((-1e30, -1e-30, -3), (1e30, 1e-30, 5), (7, 1000, 3)), ((1, 1, 1), tuple(np.nextafter(np.float32(1), np.float32(2)).repeat(3)), (2, 3, 5))]
    for _ in range(200):
        centre = rng.normal(size=3) * 10.0 ** rng.integers(-3, 4)
        half = 10.0 ** rng.uniform(-4, 4, size=3)
        lo, hi = (centre - half).astype(np.float32), (centre + half).astype(np.float32)
        if (lo < hi).all():
            cases.append((lo, hi, tuple(int(x) for x in rng.integers(2, 1025, size=3))))
    for lo, hi, n in cases:
        g = ms.grid_of(lo, hi, n, 16)
        got = np.array(wl.mesh_grid_check(g), dtype=np.float32)
        assert got.tobytes() == ms.np_h(lo, hi, n).tobytes(), (lo, hi, n)
        corners = (n[0] + 1) * (n[1] + 1) * (n[2] + 1)
        need = wl.mesh_scratch_bytes(g)
        assert need > 12 * corners and need % 16 == 0
    assert wl.mesh_grid_check(ms.grid_of((-2, -2, -2), (2, 2, 2), (32, 32, 32), 16)) == [0.125, 0.125, 0.125]
    assert wl.mesh_grid(( -1, -1, -1), (1, 1, 1), 5).n[:] == [5, 5, 5]


def test_mesh_without_device_fails_loudly(hostonly):
    r = wl.Renderer("nodev", max_nodes=4)
    if r.lib.wo_renderer_device(r.ptr) != -1:
        r.close()
        pytest.skip("this machine has a HIP device: the made-up addresses below must never reach one")
    r.sphere(1.0)
    g = _grid()
    need = wl.mesh_scratch_bytes(g)
    for call in (lambda: r.mesh_device(g, 0x1000, 8, 0x2000, 0x3000, 8, 0x4000, 0x5000, need), lambda: r.mesh(g),
                 lambda: r.mesh_device(g, 0, 0, 0, 0, 0, 0x4000, 0x5000, need)):
        wl.clear_error()
        with pytest.raises(wl.WololoError, match="device"):
            call()
    # bad arguments are refused before that, each by its own message
    bad = _grid(iters=25)
    for text, call in (("bisection steps", lambda: r.mesh(bad)),
                       ("bisection steps", lambda: r.mesh_device(bad, 0x1000, 8, 0x2000, 0, 8, 0x4000, 0x5000, need)),
                       ("NULL grid", lambda: r.mesh_device(None, 0x1000, 8, 0x2000, 0, 8, 0x4000, 0x5000, need)),
                       ("NULL counts", lambda: r.mesh_device(g, 0x1000, 8, 0x2000, 0, 8, 0, 0x5000, need)),
                       ("NULL scratch", lambda: r.mesh_device(g, 0x1000, 8, 0x2000, 0, 8, 0x4000, 0, need)),
                       ("NULL vertex", lambda: r.mesh_device(g, 0, 8, 0x2000, 0, 8, 0x4000, 0x5000, need)),
                       ("NULL quad", lambda: r.mesh_device(g, 0x1000, 8, 0, 0, 8, 0x4000, 0x5000, need)),
                       ("16-byte aligned", lambda: r.mesh_device(g, 0x1008, 8, 0x2000, 0, 8, 0x4000, 0x5000, need)),
                       ("16-byte aligned", lambda: r.mesh_device(g, 0x1000, 8, 0x2000, 0x3004, 8, 0x4000, 0x5000, need)),
                       ("short of", lambda: r.mesh_device(g, 0x1000, 8, 0x2000, 0, 8, 0x4000, 0x5000, need - 1))):
        wl.clear_error()
        with pytest.raises(wl.WololoError, match=text) as e:
            call()
        assert "device" not in str(e.value).replace("wo_renderer_mesh_device", ""), str(e.value)
    assert r.lib.wo_renderer_mesh(r.ptr, ctypes.byref(g), None) == -1 and "NULL result" in wl.last_error()
    m = wl.Mesh()
    assert r.lib.wo_renderer_mesh(r.ptr, ctypes.byref(g), ctypes.byref(m)) == -1 and not m.vertices
    assert r.ray_path() == "none"
    r.close()


# ---- the reference, pinned to things it shares no code with ----
@pytest.mark.parametrize("scene,n,iters", CASES, ids=CASE_IDS)
def test_reference_is_closed_and_faces_outward(hostonly, scene, n, iters):
    m = ms.scene_reference(scene, n, iters)
    nv, nq, caps = m["counts"]
    print(scene, n, iters, "vertices, quads, caps", m["counts"])
    assert nq >= 100 and len(m["quads"]) == nq and len(m["vertices"]) == nv
    assert ms.directed_edge_imbalance(m["quads"]) == 0
    vol = ms.signed_volume(m["vertices"]["p"], m["quads"])
    lo, hi = (np.array(v) for v in sp.BOXES[scene])
    assert 0.0 < vol < float((hi - lo).prod()), vol
    # every vertex lies in its cell, every quad's four cells touch its edge
    h = m["h"].astype(np.float64)
    cell = m["vertices"]["cell"].astype(np.int64)
    ijk = np.stack([cell % n[0], (cell // n[0]) % n[1], cell // (n[0] * n[1])], axis=1)
    rel = (m["vertices"]["p"].astype(np.float64) - lo) / h - ijk
    assert (rel > -1e-4).all() and (rel < 1 + 1e-4).all()
    assert (np.diff(cell) > 0).all()
    assert (m["ids"]["flags"] & wl.MESH_QUAD_CAP != 0).sum() == caps
    # a quad's normal (its diagonals' cross product) points along its axis, +axis when POSITIVE
    p = m["vertices"]["p"].astype(np.float64)[m["quads"].astype(np.int64)]
    normal = np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 1])
    axis = (m["ids"]["flags"] & wl.MESH_QUAD_AXIS).astype(np.int64)
    along = normal[np.arange(nq), axis]
    positive = (m["ids"]["flags"] & wl.MESH_QUAD_POSITIVE) != 0
    assert ((along > 0) == positive).all()


def test_the_cases_keep_telling(hostonly):
    """Caps, a case without caps, and an edge shared by four quads (two sheets touching) occur."""
    by_case = {(s, n): ms.scene_reference(s, n, it) for s, n, it in CASES}
    assert all(m["counts"][2] > 0 for (s, _), m in by_case.items() if s in ("csg256_chain", "rtiow_cover"))
    assert all(m["counts"][2] == 0 for (s, _), m in by_case.items() if s == "csg32")
    assert ms.max_edge_use(by_case["csg256_chain", ms.GRIDS[1][0]]["quads"]) == 4
    assert ms.max_edge_use(by_case["csg32", ms.GRIDS[0][0]]["quads"]) == 2


@pytest.mark.parametrize("scene,n,iters", CASES, ids=CASE_IDS)
def test_reported_leaf_separates_the_bracket(hostonly, scene, n, iters):
    """For every non-cap quad the reported leaf's own test, evaluated here in float64 from the
    record, differs between the final bracket's two points; it is a WO_LEAF_* record and its node
    is wo_renderer_program_nodes' entry."""
    m = ms.scene_reference(scene, n, iters)
    r = ms.scene_renderer(scene)
    prog, nrec, _ = r.program()
    nodes = r.program_nodes()
    mats, n_mats = r.materials()
    ids = m["ids"]
    live = np.flatnonzero((ids["flags"] & wl.MESH_QUAD_CAP) == 0)
    assert len(live) >= 50
    cap = (ids["flags"] & wl.MESH_QUAD_CAP) != 0
    assert (ids["leaf"][cap] == ms.NONE).all() and (ids["node"][cap] == ms.NONE).all() and (ids["material"][cap] == ms.NONE).all()
    f32 = np.float32
    for q in live:
        leaf = int(ids["leaf"][q])
        assert leaf < nrec and prog[leaf].op in (wl.WO_LEAF_SPHERE, wl.WO_LEAF_HALFSPACE)
        assert ids["node"][q] == nodes[leaf] != wl.WO_NODE_INVALID
        assert ids["material"][q] == (prog[leaf].u0 if prog[leaf].u0 < n_mats else 0)
        f = [f32(x) for x in prog[leaf].f[:4]]
        tests = []
        for p in (m["pa"][q], m["pb"][q]):
            if prog[leaf].op == wl.WO_LEAF_SPHERE:
                g = [f32(p[a] - f[a]) for a in range(3)]
                v = f32(f32(f32(g[0] * g[0]) + f32(g[1] * g[1])) + f32(g[2] * g[2]))
            else:
                v = f32(f32(f32(f[0] * p[0]) + f32(f[1] * p[1])) + f32(f[2] * p[2]))
            tests.append(bool(v <= f[3]))
        assert tests[0] != tests[1], (scene, q, leaf)
    r.close()


def _sphere_reference(radius, half, n, iters):
    r = wl.Renderer("sphere", max_nodes=4)
    r.sphere(radius)
    prog, nrec, _ = r.program()
    m = ms.reference_mesh(prog, nrec, r.program_nodes(), r.materials()[1], (-half,) * 3, (half,) * 3, n, iters)
    r.close()
    return m


def test_sphere_vertices_lie_in_the_shell(hostonly):
    """Radius 1.5 in the box +-2 at 32^3 cells, 16 bisections: the crossings are within delta =
    h 2^-16 + 1e-6 of the surface and a cell's diagonal is h sqrt(3), so a vertex, a mean of
    crossings on its cell's edges, has a radius in [sqrt(r^2 - 3 h^2 / 4) - delta, r + delta]."""
    rad, h = 1.5, 0.125
    m = _sphere_reference(rad, 2.0, (32, 32, 32), 16)
    delta = h * 2.0 ** -16 + 1e-6
    radius = np.sqrt((m["vertices"]["p"].astype(np.float64) ** 2).sum(axis=1))
    print("sphere: vertex radii in", radius.min(), radius.max(), "bounds", np.sqrt(rad * rad - 0.75 * h * h) - delta, rad + delta)
    assert m["counts"][2] == 0 and m["counts"][1] > 1000
    assert radius.min() >= np.sqrt(rad * rad - 0.75 * h * h) - delta and radius.max() <= rad + delta
    assert ms.directed_edge_imbalance(m["quads"]) == 0
    vol = ms.signed_volume(m["vertices"]["p"], m["quads"])
    assert 0.9 * 4.0 / 3.0 * np.pi * rad ** 3 < vol < 4.0 / 3.0 * np.pi * rad ** 3


def test_large_sphere_is_all_caps(hostonly):
    """Radius 100 round the box +-1 at (4, 5, 6) cells: every interior corner is inside, every
    quad a cap and cap_quads == quads.  Every crossing lies within h 2^-iters of a face of the box
    (the bracket starts at the forced corner on the face and is halved `iters` times towards it), and
    so does the vertex of every cell in one face's layer alone, a mean of four such crossings.  A
    cell in two or three layers (along the box's edges, at its corners) averages crossings next to
    different faces, so the specification puts its vertex about h / 2 from each: those vertices are
    held to their own cell, the outermost layer."""
    iters, n = 10, (4, 5, 6)
    m = _sphere_reference(100.0, 1.0, n, iters)
    nv, nq, caps = m["counts"]
    assert nq == caps > 0 and (m["ids"]["flags"] & wl.MESH_QUAD_CAP != 0).all()
    assert nq == 2 * (3 * 4 + 3 * 5 + 4 * 5)  # the faces of the 3 x 4 x 5 block of interior corners
    p = m["vertices"]["p"].astype(np.float64)
    h = m["h"].astype(np.float64)
    tol = h * 2.0 ** -iters
    # the crossings: the middle of the final bracket, along the quad's axis
    axis = (m["ids"]["flags"] & wl.MESH_QUAD_AXIS).astype(np.int64)
    rows = np.arange(nq)
    x = 0.5 * (m["pa"].astype(np.float64)[rows, axis] + m["pb"].astype(np.float64)[rows, axis])
    assert (np.minimum(np.abs(x + 1.0), np.abs(x - 1.0)) <= tol[axis]).all()
    # the vertices, by the layers their cells lie in
    cell = m["vertices"]["cell"].astype(np.int64)
    ijk = np.stack([cell % n[0], (cell // n[0]) % n[1], cell // (n[0] * n[1])], axis=1)
    outer = (ijk == 0) | (ijk == np.array(n) - 1)
    assert outer.any(axis=1).all() and nv == 4 * 5 * 6 - 2 * 3 * 4
    dist = np.minimum(np.abs(p + 1.0), np.abs(p - 1.0))  # per coordinate, to the nearer face
    one = outer.sum(axis=1) == 1
    print("large sphere: worst distance of a one-layer vertex / its bound", (dist[one][outer[one]] / np.broadcast_to(tol, dist.shape)[one][outer[one]]).max())
    assert one.sum() == 2 * (2 * 3 + 2 * 4 + 3 * 4) and (dist[one][outer[one]] <= np.broadcast_to(tol, dist.shape)[one][outer[one]]).all()
    assert (dist[outer] <= np.broadcast_to(h, dist.shape)[outer] * (1 + 1e-6)).all()
    assert ms.directed_edge_imbalance(m["quads"]) == 0 and ms.signed_volume(p, m["quads"]) > 0


def test_empty_scene_has_no_mesh(hostonly):
    r = wl.Renderer("empty", max_nodes=4)
    prog, nrec, _ = r.program()
    assert nrec == 0
    m = ms.reference_mesh(prog, nrec, r.program_nodes(), r.materials()[1], (-1, -1, -1), (1, 1, 1), (4, 5, 6), 8)
    assert m["counts"] == (0, 0, 0) and len(m["vertices"]) == 0 and m["quads"].shape == (0, 4)
    r.close()


# ---- the OBJ writer ----
def test_obj_round_trip(hostonly, tmp_path):
    m = ms.scene_reference("csg256_chain", *ms.GRIDS[0])
    path = str(tmp_path / "chain.obj")
    wl.write_obj(path, m["vertices"], m["quads"], m["ids"])
    verts, groups = ms.parse_obj(path)
    assert verts.tobytes() == np.ascontiguousarray(m["vertices"]["p"]).tobytes()  # %.9g: the floats' bits
    cap = (m["ids"]["flags"] & wl.MESH_QUAD_CAP) != 0
    nodes = sorted(set(int(x) for x in m["ids"]["node"][~cap]))
    assert [g for g, _ in groups] == [f"node_{x}" for x in nodes] + ["cap"] and len(nodes) >= 2
    for name, faces in groups:
        want = m["quads"][cap] if name == "cap" else m["quads"][~cap & (m["ids"]["node"] == int(name[5:]))]
        assert faces.tobytes() == np.ascontiguousarray(want).tobytes(), name  # quad order kept inside a group
    # without ids: one list, in order
    wl.write_obj(path, m["vertices"], m["quads"])
    verts, groups = ms.parse_obj(path)
    assert len(groups) == 1 and groups[0][0] == "" and groups[0][1].tobytes() == m["quads"].tobytes()
    assert ms.directed_edge_imbalance(groups[0][1]) == 0
    with pytest.raises(wl.WololoError, match="names vertex"):
        wl.write_obj(path, m["vertices"][:-1], m["quads"])
    with pytest.raises(wl.WololoError, match="cannot open"):
        wl.write_obj(str(tmp_path / "no" / "such" / "dir.obj"), m["vertices"], m["quads"])


def test_mesh_driver_runs_clean_under_sanitizers():
    """csrc/mesh.c with tests/host/mesh_main.c (its own main), built with ASan + UBSan."""
    run = subprocess.run(["make", "-C", CSRC, "mesh-asan"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "mesh driver: ok" in run.stdout and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr
