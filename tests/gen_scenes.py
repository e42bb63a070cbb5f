"""Seeded CSG scene families for the tests (a plain helper module: no fixtures, no plugin).

Every builder makes its scene through the public wl.Renderer calls and mirrors it in
`Shadow`, a float64 point classifier over the node tables that shares no code with the
scene compiler, the oracle or the kernels.  `build(r, family, n_leaves, seed, **knobs)`
is deterministic in its arguments.

Families (build's `family`):
  random    random pairing of a pool of leaves (as `_random_scene`), knobs `roots` (stop
            with that many roots: the scene is then the balanced union of them) and
            `reuse` (that many merged operands stay in the pool: the tree is a DAG)
  balanced  paired level by level
  chain     left-deep
  pairs     a balanced union of two-leaf terms `a op b`; `exact=True` takes only
            union / difference over spheres, so primitives == leaves
  ties      coincident and tangent surfaces (equal event keys), unioned; `extra=k` adds k
            pair terms, `nest=True` folds the items with alternating difference /
            intersection instead

Unbounded half-spaces only ever cut a sphere (sphere & half-space, sphere \\ half-space),
so every solid is bounded and a camera a few units away is outside it (the CPU tests
still ask the classifier).  Operands are rotated by a random quaternion with probability
1/2; leaf materials cycle over Lambertian, mirror metal, fuzzy metal and glass.
"""
import math
import re

import numpy as np

from csgrenderer_amd import wololo as wl


class Shadow:
    """Records nodes as they are added through the C API."""

    def __init__(self, r: wl.Renderer):
        self.r = r
        self.nodes = []
        self.nonroot = set()
        self.mats = None

    def paint(self):
        """From here on every new leaf takes the next of four materials."""
        r = self.r
        self.mats = [r.lambertian((0.7, 0.4, 0.3)), r.metal((0.9, 0.9, 0.9), 0.0), r.metal((0.8, 0.7, 0.5), 0.3),
                     r.dielectric(1.5)]
        self.n_painted = 0

    def _leaf(self, n):
        if self.mats:
            self.r.set_material(n, self.mats[self.n_painted % len(self.mats)])
            self.n_painted += 1
        return n

    def sphere(self, rad):
        n = self.r.sphere(rad)
        self.nodes.append(("s", rad))
        return self._leaf(n)

    def halfspace(self, nrm):
        n = self.r.halfspace(nrm)
        self.nodes.append(("h", np.array(nrm, dtype=np.float64)))
        return self._leaf(n)

    def binop(self, op, a, b):
        fn = {"u": self.r.union, "i": self.r.intersection, "d": self.r.difference}[op]
        n = fn(a, b)
        self.nodes.append((op, a, b))
        self.nonroot.update([a.node, b.node])
        return n

    def roots(self):
        return [i for i in range(len(self.nodes)) if i not in self.nonroot]

    # ---- float64 point classification ----
    @staticmethod
    def _rotation(arg):
        q = arg.orientation
        w, x, y, z = q.real, q.imaginary.x, q.imaginary.y, q.imaginary.z
        nq = math.sqrt(w * w + x * x + y * y + z * z)
        w, x, y, z = (1.0, 0.0, 0.0, 0.0) if nq == 0 else (w / nq, x / nq, y / nq, z / nq)
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                         [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])

    @classmethod
    def _to_local(cls, arg, p):
        off = np.array([arg.offset.x, arg.offset.y, arg.offset.z])
        return cls._rotation(arg).T @ (p - off)

    def inside(self, node, p):
        nd = self.nodes[node]
        if nd[0] == "s":
            return float(np.dot(p, p)) <= abs(nd[1]) ** 2
        if nd[0] == "h":
            n = nd[1]
            ln = np.linalg.norm(n)
            return True if ln == 0 else float(np.dot(n / ln, p)) <= 0.0
        a = self.inside(nd[1].node, self._to_local(nd[1], p))
        b = self.inside(nd[2].node, self._to_local(nd[2], p))
        return {"u": a or b, "i": a and b, "d": a and not b}[nd[0]]

    def scene_inside(self, p):
        return any(self.inside(i, p) for i in range(len(self.nodes)) if i not in self.nonroot)

    # the same classification for an (n, 3) array of points at once (float64 throughout)
    def inside_many(self, node, P):
        nd = self.nodes[node]
        if nd[0] == "s":
            return (P * P).sum(axis=1) <= abs(nd[1]) ** 2
        if nd[0] == "h":
            ln = np.linalg.norm(nd[1])
            return np.ones(len(P), dtype=bool) if ln == 0 else P @ (nd[1] / ln) <= 0.0
        vals = []
        for arg in nd[1:3]:
            off = np.array([arg.offset.x, arg.offset.y, arg.offset.z])
            vals.append(self.inside_many(arg.node, (P - off) @ self._rotation(arg)))  # rows of R^T (p - off)
        a, b = vals
        return {"u": a | b, "i": a & b, "d": a & ~b}[nd[0]]

    def scene_inside_many(self, P):
        P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
        out = np.zeros(len(P), dtype=bool)
        for i in self.roots():
            out |= self.inside_many(i, P)
        return out


def _rand_quat(rng):
    v = rng.normal(size=4)
    v /= np.linalg.norm(v)
    return wl.Quaternion(v[0], wl.Vec3(v[1], v[2], v[3]))


def _random_scene(seed, n_leaves=10, axis=False):
    """axis=True: half-space normals are +-e_a and operands are only translated, so
    the compiled leaves are axis-aligned (u1 != 0) and take the reciprocal path."""
    rng = np.random.default_rng(seed)
    r = wl.Renderer(f"rand{seed}", max_nodes=256)
    sh = Shadow(r)
    pool = []
    for _ in range(n_leaves):
        if rng.random() < 0.7:
            pool.append(sh.sphere(rng.uniform(0.4, 1.2)))
        else:
            nrm = np.eye(3)[rng.integers(3)] * rng.choice([-1.0, 1.0]) if axis else rng.normal(size=3)
            pool.append(sh.halfspace(nrm))
    while len(pool) > 1:
        i, j = rng.choice(len(pool), 2, replace=False)
        a, b = pool[i], pool[j]
        op = rng.choice(["u", "i", "d"], p=[0.45, 0.3, 0.25])
        mk = lambda n: wl.arg(n, tuple(rng.uniform(-1.0, 1.0, 3)),
                              _rand_quat(rng) if rng.random() < 0.5 and not axis else None)
        n = sh.binop(op, mk(a), mk(b))
        pool = [x for k, x in enumerate(pool) if k not in (i, j)] + [n]
    return r, sh, rng


# ---- the families ------------------------------------------------------------------------------

def _place(rng, node, spread=1.0):
    """The node as an operand: a random offset, and with probability 1/2 a random rotation."""
    off = tuple(float(v) for v in rng.uniform(-spread, spread, 3))
    return wl.arg(node, off, _rand_quat(rng) if rng.random() < 0.5 else None)


def _pool(sh, rng, n_leaves, halfspaces=0.25, carve=0.4, rad=(0.4, 1.1)):
    """Bounded atoms that use exactly n_leaves leaves: a sphere, or (two leaves) a sphere cut
    by a rotated half-space through a point near its centre: carved away with probability
    `carve`, else kept (an intersection: one two-member primitive)."""
    pool, left = [], n_leaves
    while left > 0:
        s = sh.sphere(float(rng.uniform(*rad)))
        left -= 1
        if left > 0 and rng.random() < halfspaces:
            h = sh.halfspace(tuple(float(v) for v in rng.normal(size=3)))
            left -= 1
            s = sh.binop("i" if rng.random() < 1.0 - carve else "d", wl.arg(s), _place(rng, h, 0.3))
        pool.append(s)
    return pool


def _op(rng, ops):
    return str(rng.choice(["u", "i", "d"], p=ops))


def _balanced_union(sh, rng, items, spread):
    while len(items) > 1:
        nxt = [sh.binop("u", _place(rng, items[i], spread), _place(rng, items[i + 1], spread))
               for i in range(0, len(items) - 1, 2)]
        if len(items) % 2:
            nxt.append(items[-1])
        items = nxt
    return items[0]


def _random(sh, rng, n, ops=(0.45, 0.3, 0.25), halfspaces=0.25, carve=0.4, roots=1, reuse=0, spread=1.0):
    pool = _pool(sh, rng, n, halfspaces, carve)
    while len(pool) > roots:
        i, j = (int(v) for v in rng.choice(len(pool), 2, replace=False))
        node = sh.binop(_op(rng, ops), _place(rng, pool[i], spread), _place(rng, pool[j], spread))
        drop = {i, j}
        if reuse > 0 and len(pool) > roots + 1:
            drop.discard(i)  # pool[i] stays: an operand again later, one node in two places
            reuse -= 1
        pool = [x for k, x in enumerate(pool) if k not in drop] + [node]


def _balanced(sh, rng, n, ops=(0.45, 0.3, 0.25), halfspaces=0.25, carve=0.4, spread=1.0):
    items = _pool(sh, rng, n, halfspaces, carve)
    while len(items) > 1:
        nxt = [sh.binop(_op(rng, ops), _place(rng, items[i], spread), _place(rng, items[i + 1], spread))
               for i in range(0, len(items) - 1, 2)]
        if len(items) % 2:
            nxt.append(items[-1])
        items = nxt


def _chain(sh, rng, n, ops=(0.5, 0.1, 0.4), halfspaces=0.25, carve=0.4, spread=1.0):
    pool = _pool(sh, rng, n, halfspaces, carve)
    acc = pool[0]
    for x in pool[1:]:
        acc = sh.binop(_op(rng, ops), _place(rng, acc, 0.15 * spread), _place(rng, x, spread))


def _pair_terms(sh, rng, n, exact, halfspaces):
    """Two-leaf terms `a op b` over n leaves (a lone sphere when n is odd)."""
    terms = []
    for k in range(n // 2):
        a = sh.sphere(float(rng.uniform(0.4, 0.8)))
        if not exact and rng.random() < halfspaces:
            b = sh.halfspace(tuple(float(v) for v in rng.normal(size=3)))
            op = "id"[k % 2]
        else:
            b = sh.sphere(float(rng.uniform(0.3, 0.7)))
            op = "ud"[k % 2] if exact else "udi"[k % 3]
        terms.append(sh.binop(op, wl.arg(a), _place(rng, b, 0.4)))
    if n % 2:
        terms.append(sh.sphere(float(rng.uniform(0.4, 0.8))))
    return terms


def _pairs(sh, rng, n, exact=False, halfspaces=0.25, spread=1.2):
    _balanced_union(sh, rng, _pair_terms(sh, rng, n, exact, halfspaces), spread)


def _tie_items(sh):
    """The degenerate constructions, each about one unit across: (node, leaves)."""
    A = wl.arg
    items = []
    a, a2 = sh.sphere(0.7), sh.sphere(0.7)
    items.append(sh.binop("d", A(a), A(a2)))                         # a \ a': empty, four equal keys per ray
    b = sh.sphere(0.65)
    items.append(sh.binop("u", A(b), A(b)))                          # a u a: one node instanced twice
    c, c2 = sh.sphere(0.7), sh.sphere(0.7)
    items.append(sh.binop("i", A(c), A(c2)))                         # a & a': one primitive, equal members
    d, d2 = sh.sphere(0.7), sh.sphere(0.35)
    items.append(sh.binop("d", A(d), A(d2, (0.35, 0.0, 0.0))))       # internally tangent, carved
    e, e2 = sh.sphere(0.4), sh.sphere(0.4)
    items.append(sh.binop("u", A(e, (-0.4, 0.0, 0.0)), A(e2, (0.4, 0.0, 0.0))))  # externally tangent
    f, up, down = sh.sphere(0.7), sh.halfspace((0.0, 1.0, 0.0)), sh.halfspace((0.0, -1.0, 0.0))
    slab = sh.binop("i", A(up), A(down))                             # zero thickness: the plane y = 0
    items.append(sh.binop("u", A(sh.binop("i", A(f), A(slab))), A(sh.sphere(0.3), (0.0, 0.5, 0.0))))
    g, cut = sh.sphere(0.7), sh.halfspace((0.3, 1.0, 0.2))
    items.append(sh.binop("i", A(g), A(cut)))                        # a hemisphere cut through its centre
    h, h2 = sh.sphere(0.7), sh.sphere(0.7)
    items.append(sh.binop("u", A(h), A(h2)))                         # a u a': two nodes, one surface
    return items


def _ties(sh, rng, n, extra=0, nest=False, spread=1.6):
    """`n` does not size the construction (its leaves are fixed); `extra` pair terms of two
    spheres each join the union, behind the items."""
    items = _tie_items(sh)
    if nest:
        # ((((B \\ i0) & (C u i1)) \\ i2) & (C u i3)) ...: C (one node in many places: a DAG)
        # keeps the intersections from emptying the solid
        big, keep = sh.sphere(2.2), sh.sphere(1.9)
        acc = big
        for k, it in enumerate(items):
            where = _place(rng, it, 1.1)
            if k % 2 == 0:
                acc = sh.binop("d", wl.arg(acc), where)
            else:
                acc = sh.binop("i", wl.arg(acc), wl.arg(sh.binop("u", _place(rng, keep, 0.2), where)))
    else:
        # a 3 x 3 grid facing +z, so that no item hides another; each item turned at random
        cells = [wl.arg(it, (spread * (k % 3 - 1), spread * (k // 3 - 1), 0.0),
                        _rand_quat(rng) if rng.random() < 0.5 else None) for k, it in enumerate(items)]
        while len(cells) > 1:
            nxt = [wl.arg(sh.binop("u", cells[i], cells[i + 1])) for i in range(0, len(cells) - 1, 2)]
            if len(cells) % 2:
                nxt.append(cells[-1])
            cells = nxt
        acc = cells[0].node
    if extra:
        more = _balanced_union(sh, rng, _pair_terms(sh, rng, 2 * extra, True, 0.0), 1.0)
        sh.binop("u", wl.arg(acc), wl.arg(more, (0.0, 0.0, -2.5)))


FAMILIES = {"random": _random, "balanced": _balanced, "chain": _chain, "pairs": _pairs, "ties": _ties}


def build(r, family, n_leaves, seed, **knobs):
    """Build the scene into renderer `r` (empty before); returns its Shadow."""
    rng = np.random.default_rng(seed)
    sh = Shadow(r)
    sh.paint()
    FAMILIES[family](sh, rng, n_leaves, **knobs)
    return sh


# ---- what a compiled scene is, as facts read from its generated source and lane BVH ------------

MARKERS = {"term": "// term mode:", "ucount": "kUTerm", "dl": "decision list", "lut": "#define WO_JIT_LUT 1\n",
           "hlut": "#define WO_JIT_HLUT 1\n"}


def forms(src):
    """The root-evaluation forms a generated source names ("flat": none of them)."""
    got = {k for k, text in MARKERS.items() if text in src}
    return frozenset(got or {"flat"})


def define(src, name):
    """The value of the source's own `#define name <int>` (None when it has none)."""
    m = re.search(r"^#define " + name + r" (\d+)", src, re.M)
    return int(m.group(1)) if m else None


def lut_subtrees(src):
    """How many truth tables the root splits into (0 without them)."""
    m = re.search(r"^// root by truth tables: (\d+) subtrees", src, re.M)
    return int(m.group(1)) if m else 0


def describe(r):
    """Facts about the renderer's compiled scene (no device needed)."""
    prog, nrec, nprim = r.program()
    src = r.jit_source() or ""
    mats, nm = r.materials()
    d = wl.lane_bvh(prog, nrec, nprim, mats, nm)[0]
    ops = [prog[i].op for i in range(nrec)]
    kind = 14 if d.wide else 6 if d.terms else 7 if d.general else 3 if d.spheres_only else 2
    return {"nprim": nprim, "nrec": nrec, "forms": forms(src), "words": (nprim + 31) // 32,
            "lds_prog": define(src, "WO_JIT_LDS_PROG"), "hbits_lds": define(src, "WO_HBITS_LDS"),
            "window": define(src, "WO_WINDOW"), "rdiff": ops.count(wl.WO_OP_RDIFF), "bound": ops.count(wl.WO_OP_BOUND),
            "lut_subtrees": lut_subtrees(src),
            "lane": {"terms": d.terms, "general": d.general, "union_only": d.union_only,
                     "spheres_only": d.spheres_only, "gwords": d.gwords, "kind": kind}}
