"""Shared by tests/test_mesh.py and tests/test_gpu_mesh.py (test helper, no fixture): the numpy
restatement of renderer_ext.h's "surface mesh of the solid" (naive surface nets on a uniform
grid), built on span_support.classify_points_f32, and what the tests judge a mesh by: the
directed-edge balance, the signed volume by the divergence theorem in float64, an OBJ parser."""
import numpy as np

import span_support as sp
from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl

VERTEX_DT = np.dtype(wl.MESH_VERTEX_FIELDS)
IDS_DT = np.dtype(wl.MESH_QUAD_IDS_FIELDS)
NONE = 0xFFFFFFFF
# the parity cases: every scene at both grids
SCENES = ["csg32", "csg32_nested", "csg256_chain", "rtiow_cover"]
GRIDS = [((13, 7, 11), 12), ((67, 21, 45), 16)]
SENTINEL = sp.SENTINEL


def grid_of(lo, hi, n, iters, flags=0, reserved=0):
    g = wl.MeshGrid()
    g.lo[:] = [float(np.float32(x)) for x in lo]
    g.hi[:] = [float(np.float32(x)) for x in hi]
    g.n[:] = [int(x) for x in n]
    g.iters, g.flags, g.reserved = int(iters), int(flags), int(reserved)
    return g


def np_h(lo, hi, n):
    """h[a] = (hi[a] - lo[a]) / (float)n[a]: a difference, then a correctly rounded division."""
    lo, hi = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
    return ((hi - lo) / np.asarray(n, dtype=np.uint32).astype(np.float32)).astype(np.float32)


def scene_renderer(scene):
    r = wl.Renderer(scene, max_nodes=4096)
    scenes.build(scene, r)
    r.set_tracer("interpreter")
    return r


def leaf_tests_differ(prog, nrec, Pa, Pb):
    """Per pair of points the first leaf record, in program order, whose own test (v <= f[3], as
    classify_points_f32 evaluates it) differs between them; NONE where no leaf's does."""
    first = np.full(len(Pa), NONE, dtype=np.uint32)

    def test(L, P):
        f = np.array(L.f[:4], dtype=np.float32)
        px, py, pz = P[:, 0], P[:, 1], P[:, 2]
        if L.op == wl.WO_LEAF_SPHERE:
            gx, gy, gz = px - f[0], py - f[1], pz - f[2]
            q = (gx * gx + gy * gy) + gz * gz
        else:
            q = (f[0] * px + f[1] * py) + f[2] * pz
        assert q.dtype == np.float32
        return q <= f[3]

    for pc in range(nrec):
        L = prog[pc]
        if L.op not in (wl.WO_LEAF_SPHERE, wl.WO_LEAF_HALFSPACE):
            continue
        d = (test(L, Pa) != test(L, Pb)) & (first == NONE)
        first[d] = pc
    return first


def reference_mesh(prog, nrec, nodes, n_mats, lo, hi, n, iters):
    """The specification, step by step.  Returns a dict: vertices (VERTEX_DT), quads (Q, 4) uint32,
    ids (IDS_DT), counts (vertices, quads, cap_quads), and for the tests' own use ta, tb (the
    final bracket of every quad's edge as (Q, 3) points) and inside (the corner bits, [k, j, i])."""
    f32 = np.float32
    lo, hi = np.asarray(lo, dtype=f32), np.asarray(hi, dtype=f32)
    n = [int(x) for x in n]
    h = np_h(lo, hi, n)
    N = [x + 1 for x in n]
    coord = [(lo[a] + np.arange(N[a], dtype=np.uint32).astype(f32) * h[a]).astype(f32) for a in range(3)]
    K, J, I = np.meshgrid(np.arange(N[2]), np.arange(N[1]), np.arange(N[0]), indexing="ij")
    P = np.stack([coord[0][I], coord[1][J], coord[2][K]], axis=-1).reshape(-1, 3)
    plain = sp.classify_points_f32(prog, nrec, P).reshape(N[2], N[1], N[0])
    interior = (I > 0) & (I < n[0]) & (J > 0) & (J < n[1]) & (K > 0) & (K < n[2])
    inside = plain & interior

    def shifted(arr, a):  # the value at C + e_a, over the lower corners C of the edges along a
        sl = [slice(None)] * 3
        sl[2 - a] = slice(1, None)
        return arr[tuple(sl)]

    def lower(arr, a):
        sl = [slice(None)] * 3
        sl[2 - a] = slice(0, -1)
        return arr[tuple(sl)]

    # the taken edges, ordered by (corner number of the lower corner) * 3 + a
    keys, axes, cidx = [], [], []
    for a in range(3):
        taken = lower(inside, a) != shifted(inside, a)
        k, j, i = np.nonzero(taken)
        corner = (k * N[1] + j) * N[0] + i
        keys.append(corner * 3 + a)
        axes.append(np.full(len(corner), a))
        cidx.append(np.stack([i, j, k], axis=1))
    keys, axes, cidx = np.concatenate(keys), np.concatenate(axes), np.concatenate(cidx)
    order = np.argsort(keys, kind="stable")
    keys, axes, cidx = keys[order], axes[order], cidx[order]
    Q = len(keys)
    rows = np.arange(Q)
    base = np.stack([coord[0][cidx[:, 0]], coord[1][cidx[:, 1]], coord[2][cidx[:, 2]]], axis=1).astype(f32)
    sa = inside[cidx[:, 2], cidx[:, 1], cidx[:, 0]]
    ta = base[rows, axes].copy()
    up = cidx.copy()
    up[rows, axes] += 1
    tb = np.stack([coord[0][up[:, 0]], coord[1][up[:, 1]], coord[2][up[:, 2]]], axis=1).astype(f32)[rows, axes]
    half = f32(0.5)
    for _ in range(iters):
        tm = (half * (ta + tb)).astype(f32)
        pm = base.copy()
        pm[rows, axes] = tm
        same = sp.classify_points_f32(prog, nrec, pm) == sa
        ta = np.where(same, tm, ta)
        tb = np.where(same, tb, tm)
    x = (half * (ta + tb)).astype(f32)
    pa, pb = base.copy(), base.copy()
    pa[rows, axes] = ta
    pb[rows, axes] = tb
    A = sp.classify_points_f32(prog, nrec, pa) if Q else np.zeros(0, bool)
    B = sp.classify_points_f32(prog, nrec, pb) if Q else np.zeros(0, bool)
    cap = A == B
    leaf = leaf_tests_differ(prog, nrec, pa, pb)
    assert (leaf[~cap] != NONE).all(), "the root differs but no leaf test does"
    ids = np.zeros(Q, dtype=IDS_DT)
    ids["leaf"] = np.where(cap, NONE, leaf)
    safe = np.where(cap, 0, leaf).astype(np.int64)
    nodes = np.asarray(nodes, dtype=np.uint32)
    mat = np.array([prog[int(pc)].u0 for pc in safe], dtype=np.uint32) if Q else np.zeros(0, np.uint32)
    ids["node"] = np.where(cap, NONE, nodes[safe] if len(nodes) else 0)
    ids["material"] = np.where(cap, NONE, np.where(mat < n_mats, mat, 0))
    ids["flags"] = axes.astype(np.uint32) | np.where(sa, wl.MESH_QUAD_POSITIVE, 0).astype(np.uint32) | \
        np.where(cap, wl.MESH_QUAD_CAP, 0).astype(np.uint32)

    # the crossing of every taken edge, by lower corner and axis
    cross = [np.zeros((N[2], N[1], N[0]), dtype=f32) for _ in range(3)]
    took = [np.zeros((N[2], N[1], N[0]), dtype=bool) for _ in range(3)]
    for a in range(3):
        m = axes == a
        cross[a][cidx[m, 2], cidx[m, 1], cidx[m, 0]] = x[m]
        took[a][cidx[m, 2], cidx[m, 1], cidx[m, 0]] = True

    # vertices: one per active cell, by cell number; the sum in the fixed order
    ck, cj, ci = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    ck, cj, ci = ck.reshape(-1), cj.reshape(-1), ci.reshape(-1)
    cell = [ci, cj, ck]
    total = np.zeros((len(ci), 3), dtype=f32)
    count = np.zeros(len(ci), dtype=np.uint32)
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        for dv in (0, 1):
            for du in (0, 1):
                e = [None] * 3
                e[a], e[u], e[v] = cell[a], cell[u] + du, cell[v] + dv
                t = took[a][e[2], e[1], e[0]]
                pt = np.zeros((len(ci), 3), dtype=f32)
                pt[:, a] = cross[a][e[2], e[1], e[0]]
                pt[:, u] = coord[u][e[u]]
                pt[:, v] = coord[v][e[v]]
                total = np.where(t[:, None], (total + pt).astype(f32), total)
                count += t
    active = count > 0
    cells = np.flatnonzero(active)
    vertices = np.zeros(len(cells), dtype=VERTEX_DT)
    vertices["p"] = (total[active] / count[active].astype(f32)[:, None]).astype(f32)
    vertices["cell"] = cells
    vindex = np.full(len(ci), NONE, dtype=np.uint32)
    vindex[cells] = np.arange(len(cells), dtype=np.uint32)

    quads = np.zeros((Q, 4), dtype=np.uint32)
    u, v = (axes + 1) % 3, (axes + 2) % 3
    for slot, (ou, ov) in enumerate(((-1, -1), (0, -1), (0, 0), (-1, 0))):
        c = cidx.copy()
        c[rows, u] += ou
        c[rows, v] += ov
        assert Q == 0 or ((c >= 0).all() and (c < np.array(n)).all()), "a quad's cell is outside the grid"
        quads[:, slot] = vindex[(c[:, 2] * n[1] + c[:, 1]) * n[0] + c[:, 0]]
    assert (quads != NONE).all()
    quads = np.where(sa[:, None], quads, quads[:, ::-1]).astype(np.uint32)
    return {"vertices": vertices, "quads": np.ascontiguousarray(quads), "ids": ids,
            "counts": (len(cells), Q, int(cap.sum())), "pa": pa, "pb": pb, "inside": inside, "h": h}


_REF = {}


def scene_reference(scene, n, iters, box=None):
    """The reference mesh of a scenes.py scene in its span_support.BOXES box: made once, shared,
    read-only."""
    key = (scene, tuple(n), iters, box)
    if key not in _REF:
        r = scene_renderer(scene)
        prog, nrec, _ = r.program()
        nodes = r.program_nodes()
        _, n_mats = r.materials()
        lo, hi = box or sp.BOXES[scene]
        m = reference_mesh(prog, nrec, nodes, n_mats, lo, hi, n, iters)
        r.close()
        for k in ("vertices", "quads", "ids", "pa", "pb", "inside"):
            m[k].setflags(write=False)
        _REF[key] = m
    return _REF[key]


def directed_edge_imbalance(quads):
    """How many directed edges p->q of the quads do not occur exactly as often as q->p."""
    q = np.asarray(quads, dtype=np.int64)
    if len(q) == 0:
        return 0
    a = q.reshape(-1)
    b = np.roll(q, -1, axis=1).reshape(-1)
    big = int(q.max()) + 1
    fwd, nf = np.unique(a * big + b, return_counts=True)
    rev, nr = np.unique(b * big + a, return_counts=True)
    if len(fwd) != len(rev) or (fwd != rev).any():
        return int(len(np.setxor1d(fwd, rev))) or 1
    return int((nf != nr).sum())


def max_edge_use(quads):
    """The most quads that share one undirected edge (2 on a manifold, 4 where two sheets touch)."""
    q = np.asarray(quads, dtype=np.int64)
    a, b = q.reshape(-1), np.roll(q, -1, axis=1).reshape(-1)
    big = int(q.max()) + 1
    _, cnt = np.unique(np.minimum(a, b) * big + np.maximum(a, b), return_counts=True)
    return int(cnt.max())


def signed_volume(p, quads):
    """The volume enclosed by the quads, each split into two triangles, by the divergence theorem
    (the sum of det(p0, p1, p2) / 6) in float64; positive for an outward-facing closed surface."""
    P = np.asarray(p, dtype=np.float64)
    q = np.asarray(quads, dtype=np.int64)
    vol = 0.0
    for tri in ((0, 1, 2), (0, 2, 3)):
        a, b, c = (P[q[:, t]] for t in tri)
        vol += float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum()) / 6.0
    return vol


def parse_obj(path):
    """(vertices (n, 3) float32 as '%.9g' round-trips them, [(group name, faces (m, 4) 0-based)])."""
    verts, groups = [], []
    with open(path) as fh:
        for line in fh:
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            if w[0] == "v":
                verts.append([np.float32(x) for x in w[1:4]])
            elif w[0] == "g":
                groups.append((w[1], []))
            elif w[0] == "f":
                if not groups:
                    groups.append(("", []))
                groups[-1][1].append([int(x) - 1 for x in w[1:5]])
    return (np.array(verts, dtype=np.float32).reshape(-1, 3),
            [(name, np.array(f, dtype=np.uint32).reshape(-1, 4)) for name, f in groups])
