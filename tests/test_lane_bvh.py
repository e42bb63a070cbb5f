"""The lane tracer's BVH builder (csrc/lane_bvh_build.cpp) on the CPU: the descriptor and
the packed blob of wo_lane_bvh_build, decoded through the descriptor's offsets (csrc/lane_bvh.h)
and checked for what the kernels rely on -- every ordinal reachable exactly once, boxes
that contain what lies below them, breadth-first node order, the stack depth, the layout.
Invariants only: the blob's bytes depend on the C++ library's partition order."""
import math

import numpy as np
import pytest

from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl

K_LEAF, K_NOREF, K_NOREF16 = 0x80000000, 0xFFFFFFFF, 0xFFFF  # lane_bvh.h
K_LITNEG, K_NOLIT, K_TERM_REC_F4 = 0x80000000, 0xFFFFFFFF, 5
K_GREF_BITS, K_GREF_MASK = 15, 0x7FFF
INF = math.inf

# scene -> the lane tracer's form (wo_dev_impl.h PathKind)
FORMS = {"csg32_union": 2, "rtiow_cover": 3, "csg32": 6, "csg256_balanced": 6, "csg512_balanced": 14,
         "csg32_nested": 7}


def _union_of_terms(r, max_lits=2):
    """Restatement of lane_bvh_build.cpp extract_terms: the root is a union of terms, each
    a conjunction of at most max_lits literals (a primitive or its complement), and
    every primitive is in one term -- the lane tracer's term mode.  The terms (lists of
    (ordinal, positive)), or None."""
    prog, nrec, nprim = r.program()
    st = []
    pc = 0
    while pc < nrec:
        op = prog[pc].op
        if op == wl.WO_OP_PRIM:
            st.append(("conj", [(prog[pc].u1, True)]))
            pc += 1 + prog[pc].u0
            continue
        pc += 1
        if op == wl.WO_OP_BOUND:
            continue
        b, a = st.pop(), st.pop()
        out = ("bad", None)
        terms_of = lambda x: [x[1]] if x[0] == "conj" else x[1]
        if a[0] != "bad" and b[0] != "bad":
            if op == wl.WO_OP_UNION:
                out = ("union", terms_of(a) + terms_of(b))
            elif op == wl.WO_OP_INTER and a[0] == b[0] == "conj":
                out = ("conj", a[1] + b[1])
            elif op in (wl.WO_OP_DIFF, wl.WO_OP_RDIFF):
                keep, sub = (a, b) if op == wl.WO_OP_DIFF else (b, a)
                singles = terms_of(sub)
                if keep[0] == "conj" and all(len(t) == 1 and t[0][1] for t in singles):
                    out = ("conj", keep[1] + [(t[0][0], False) for t in singles])
        st.append(out)
    if len(st) != 1 or st[0][0] == "bad":
        return None
    terms = [st[0][1]] if st[0][0] == "conj" else st[0][1]
    ords = [o for t in terms for o, _ in t]
    return terms if all(1 <= len(t) <= max_lits for t in terms) and len(ords) == len(set(ords)) else None


def _slack(lo, hi):
    return 1e-4 * (abs(lo) + abs(hi) + abs(hi - lo)) + 1e-5


class Built:
    """A program's lane BVH, decoded."""

    def __init__(self, prog, nrec, nprim, mats, nm, terms=None):
        self.prog, self.nrec, self.nprim, self.mats, self.nm, self.terms = prog, nrec, nprim, mats, nm, terms
        self.d, self.blob, self.lds, (self.lds_budget, self.depth_max) = wl.lane_bvh(prog, nrec, nprim, mats, nm)
        d = self.d
        self.u32 = np.frombuffer(self.blob, "<u4")
        self.f32 = np.frombuffer(self.blob, "<f4")
        self.node_f4 = 7 if d.wide else 4
        n = self.node_f4 * d.nodes * 4 if self.blob else 0
        self.nodes_f = self.f32[:n].reshape(-1, self.node_f4, 4)
        self.nodes_u = self.u32[:n].reshape(-1, self.node_f4, 4)
        self.geo = self.f32[n:n + 4 * nprim].reshape(-1, 4)
        self.kind = self.u32[n + 4 * nprim:n + 5 * nprim]
        self.always = [int(v) for v in self.u32[n + 5 * nprim:n + 5 * nprim + d.always]] if self.blob else []
        self.pc_of, self.binops = {}, []
        pc = 0
        while pc < nrec:
            if prog[pc].op == wl.WO_OP_PRIM:
                self.pc_of[prog[pc].u1] = pc
                pc += 1 + prog[pc].u0
            else:
                if prog[pc].op != wl.WO_OP_BOUND:
                    self.binops.append(prog[pc].op)
                pc += 1
        # what the leaves and the always list refer to
        self.n_ord = d.terms if d.terms else nprim

    def kind_of(self):
        d = self.d
        return 14 if d.wide else 6 if d.terms else 7 if d.general else 3 if d.spheres_only else 2 if d.union_only else 0

    def children(self, n):
        """(lo, hi, is_leaf, node index or ordinal) of node n's children."""
        f, u = self.nodes_f[n], self.nodes_u[n]
        out = []
        if self.d.wide:
            for c in range(4):
                r = int(u[6, c])
                assert r <= K_NOREF16
                if r != K_NOREF16:
                    out.append((f[[0, 2, 4], c], f[[1, 3, 5], c], bool(r & 0x8000), r & 0x7FFF))
        else:
            for c, (lo, hi) in enumerate(((f[0, :3], f[1, :3]), (f[2, :3], f[3, :3]))):
                r = int(u[c, 3])
                out.append((lo, hi, bool(r & K_LEAF), r & ~K_LEAF))
        return out

    def walk(self):
        """Breadth-first from the root: the internal nodes in visiting order, the leaves
        as (ordinal, lo, hi) (boxes None for a root that is a leaf)."""
        root = self.d.root
        if root == K_NOREF:
            return [], []
        if not self.d.wide and root & K_LEAF:
            return [], [(root & ~K_LEAF, None, None)]
        order, leaves = [root], []
        for n in order:  # grows while iterating
            for lo, hi, leaf, i in self.children(n):
                (leaves if leaf else order).append((i, lo, hi) if leaf else i)
        return order, leaves

    def levels(self, n):
        return 1 + max((self.levels(i) for _, _, leaf, i in self.children(n) if not leaf), default=0)

    def prim_box(self, ordinal):
        """Box of a primitive from the program, in double: sphere centre +- sqrt(f[3]),
        axis half-spaces; None when unbounded or empty."""
        pc = self.pc_of[ordinal]
        lo, hi = [-INF] * 3, [INF] * 3
        for m in range(self.prog[pc].u0):
            L = self.prog[pc + 1 + m]
            if L.op == wl.WO_LEAF_SPHERE:
                r = math.sqrt(float(L.f[3]))
                for a in range(3):
                    lo[a], hi[a] = max(lo[a], float(L.f[a]) - r), min(hi[a], float(L.f[a]) + r)
            elif L.op == wl.WO_LEAF_HALFSPACE and 1 <= L.u1 <= 3:
                a = L.u1 - 1  # s * x_a <= h
                if L.f[a] > 0.0:
                    hi[a] = min(hi[a], float(L.f[3]))
                else:
                    lo[a] = max(lo[a], -float(L.f[3]))
        if any(not math.isfinite(v) for v in lo + hi) or any(lo[a] > hi[a] for a in range(3)):
            return None
        return lo, hi


_cache = {}


def _built(name):
    """The scene's lane BVH (built once per session; call under the `hostonly` fixture)."""
    if name not in _cache:
        r = wl.Renderer(name, max_nodes=4096)
        scenes.build(name, r)
        _cache[name] = Built(*r.program(), *r.materials(), terms=_union_of_terms(r))
        r.close()
    return _cache[name]


@pytest.mark.parametrize("scene", sorted(FORMS))
def test_form_per_scene(hostonly, scene):
    b = _built(scene)
    assert b.kind_of() == FORMS[scene]
    # the 4-wide tree above 256 terms only
    assert bool(b.d.wide) == (scene == "csg512_balanced")
    if scene in ("csg256_balanced", "csg512_balanced"):
        assert (b.d.terms > 256) == bool(b.d.wide)
    assert bool(b.d.terms) == (b.terms is not None and not b.d.union_only)
    assert b.d.terms == (len(b.terms) if b.d.terms else 0)
    assert b.d.stack16 == (1 if b.d.wide or b.d.general else 0)


@pytest.mark.parametrize("scene", sorted(FORMS) + ["csg360_nested"])
def test_partition(hostonly, scene):
    """Union-only and term forms: every ordinal is a leaf ref or on the always list,
    exactly once.  General form: none twice, and an absent one cannot matter (the meet of
    its box and its relevance box, each with twice the slack, is empty; csg360_nested has
    such primitives, csg32_nested none)."""
    b = _built(scene)
    _, leaves = b.walk()
    seen = sorted([o for o, _, _ in leaves] + b.always)
    assert all(0 <= o < b.n_ord for o in seen)
    assert len(seen) == len(set(seen)), "an ordinal appears twice"
    if not b.d.general:
        assert seen == list(range(b.n_ord))
        return
    P, d = b.nprim, b.d
    nref = d.gnode_off - d.gpar_off
    gnode = [int(v) for v in b.u32[d.gnode_off:d.gnode_off + nref - P]]
    inf_box = ([-INF] * 3, [INF] * 3)
    meet = lambda x, y: ([max(p, q) for p, q in zip(x[0], y[0])], [min(p, q) for p, q in zip(x[1], y[1])])
    hull = lambda x, y: ([min(p, q) for p, q in zip(x[0], y[0])], [max(p, q) for p, q in zip(x[1], y[1])])

    def slacked(x, k):
        lo, hi = list(x[0]), list(x[1])
        for a in range(3):
            if math.isfinite(lo[a]) and math.isfinite(hi[a]):
                m = k * _slack(lo[a], hi[a])
                lo[a], hi[a] = lo[a] - m, hi[a] + m
        return lo, hi

    bnd = [b.prim_box(o) or inf_box for o in range(P)] + [inf_box] * len(gnode)
    con = [inf_box] * nref
    dec = lambda nd: (nd & K_GREF_MASK, (nd >> K_GREF_BITS) & K_GREF_MASK, nd >> 30)
    for i, nd in enumerate(gnode):  # operands before their node
        x, y, op = dec(nd)
        bnd[P + i] = (hull(bnd[x], bnd[y]), meet(bnd[x], bnd[y]), bnd[x], bnd[y])[op]
    for i in reversed(range(len(gnode))):  # a node before its operands
        x, y, op = dec(gnode[i])
        c = con[P + i]
        con[x] = meet(c, bnd[y]) if op in (1, 3) else c  # an intersection, or y AND NOT x: x gated by y
        con[y] = meet(c, bnd[x]) if op in (1, 2) else c
    for o in range(P):
        lo, hi = meet(slacked(bnd[o], 2.0), slacked(con[o], 2.0))
        assert any(lo[a] > hi[a] for a in range(3)) == (o not in seen), f"primitive {o}: in the walk iff it can matter"


@pytest.mark.parametrize("scene", sorted(FORMS))
def test_containment(hostonly, scene):
    """A child's stored box contains the boxes stored in that child's node; in the
    union-only scenes a leaf's box contains the primitive's box from the program."""
    b = _built(scene)
    order, leaves = b.walk()
    for n in order:
        for lo, hi, leaf, i in b.children(n):
            assert np.all(lo <= hi)
            if not leaf:
                for clo, chi, _, _ in b.children(i):
                    assert np.all(lo <= clo) and np.all(chi <= hi), (n, i)
    if b.d.union_only:
        assert leaves
        for o, lo, hi in leaves:
            plo, phi = b.prim_box(o)
            assert np.all(lo.astype(np.float64) <= plo) and np.all(np.asarray(phi) <= hi.astype(np.float64)), o


@pytest.mark.parametrize("scene", sorted(FORMS))
def test_shape(hostonly, scene):
    b = _built(scene)
    d = b.d
    order, leaves = b.walk()
    assert d.nodes > 0 and d.root == 0
    assert order == list(range(d.nodes)), "node indices increase in breadth-first order"
    if d.wide:
        assert d.depth == 3 * b.levels(0)
    else:
        assert d.depth == b.levels(0)
        assert d.depth <= min(math.ceil(math.log2(len(leaves))) + 6, b.depth_max)
        assert d.nodes == len(leaves) - 1
    if d.wide or d.general:  # 16-bit stack entries and node refs
        assert d.nodes < 0x8000 and b.n_ord < 0x8000
    if d.general:
        assert d.gnode_off - d.gpar_off <= K_GREF_MASK


@pytest.mark.parametrize("scene", sorted(FORMS))
def test_layout(hostonly, scene):
    """The sections in lane_bvh.h's order, without overlap, ending at the blob's size."""
    b = _built(scene)
    d, P = b.d, b.nprim
    align16 = lambda v: (v + 15) & ~15
    assert d.nprims == P and d.gP == P
    end = b.node_f4 * d.nodes * 16 + P * 16 + P * 4 + d.always * 4  # nodes, geo, kind, always
    assert d.term_off * 4 == align16(end)
    end = d.term_off * 4 + d.terms * K_TERM_REC_F4 * 16
    assert d.leaf_off == (end // 4 if d.spheres_only else 0)
    end += P * 64 if d.spheres_only else 0
    assert d.gpar_off * 4 == end
    nref = P + len(b.binops) if d.general else 0
    assert d.gnode_off == d.gpar_off + nref and d.gwords == (nref + 31) // 32
    end = align16(d.gnode_off * 4 + (nref - P if d.general else 0) * 4)
    if d.gclip_off:
        assert d.general and d.gclip_off * 4 == end
        end += 2 * P * 16
    assert len(b.blob) == end
    assert d.term_off % 4 == 0 and d.gclip_off % 4 == 0  # u32 offsets of 16-byte aligned float4
    assert d.top <= d.nodes
    assert b.lds <= b.lds_budget
    stacks = (d.depth * 256 * (2 if d.stack16 else 4) + 15) & ~15
    assert b.lds == stacks + d.top * b.node_f4 * 16 + (d.gwords * 256 * 4 if d.general else 0)
    # the inline geometry of single-sphere primitives, and their leaf table
    for o in range(P):
        pc = b.pc_of[o]
        single = b.prog[pc].u0 == 1 and b.prog[pc + 1].op == wl.WO_LEAF_SPHERE
        assert b.kind[o] == (1 if single else 0)
        if single:
            assert list(b.geo[o]) == list(b.prog[pc + 1].f)[:4]
    assert bool(d.spheres_only) == (bool(d.union_only) and all(b.kind == 1))
    if d.spheres_only:
        prog_bytes, mat_bytes = bytes(b.prog), bytes(b.mats)
        for o in range(P):
            pc, at = b.pc_of[o] + 1, d.leaf_off * 4 + o * 64
            assert b.blob[at:at + 32] == prog_bytes[32 * pc:32 * pc + 32]
            m = b.prog[pc].u0
            assert m < b.nm and b.blob[at + 32:at + 64] == mat_bytes[32 * m:32 * m + 32]


def test_general_tree_tables(hostonly):
    b = _built("csg32_nested")
    d, P = b.d, b.nprim
    nref = d.gnode_off - d.gpar_off
    gpar = [int(v) for v in b.u32[d.gpar_off:d.gpar_off + nref]]
    gnode = [int(v) for v in b.u32[d.gnode_off:d.gnode_off + nref - P]]
    ops = {wl.WO_OP_UNION: 0, wl.WO_OP_INTER: 1, wl.WO_OP_DIFF: 2, wl.WO_OP_RDIFF: 3}
    assert [nd >> 30 for nd in gnode] == [ops[o] for o in b.binops]
    for i, nd in enumerate(gnode):
        x, y = nd & K_GREF_MASK, (nd >> K_GREF_BITS) & K_GREF_MASK
        assert x < P + i and y < P + i  # operands before their node
        assert gpar[x] == gpar[y] == P + i
    assert d.groot == nref - 1 and gpar[d.groot] == K_NOREF
    assert gpar.count(K_NOREF) == 1
    if d.gclip_off:
        clip = b.f32[d.gclip_off:d.gclip_off + 8 * P].reshape(P, 2, 4)
        assert set(clip[:, 0, 3]) <= {0.0, 1.0} and np.all(clip[:, 1, 3] == 0.0)
        on = clip[:, 0, 3] == 1.0
        assert np.all(clip[on, 0, :3] <= clip[on, 1, :3])


@pytest.mark.parametrize("scene", ["csg32", "csg256_balanced", "csg512_balanced"])
def test_term_records(hostonly, scene):
    """Each term's record: its literals as the restated extract_terms gives them, the
    kind bits of the literals that are one or two spheres, and those spheres."""
    b = _built(scene)
    d = b.d
    rec_u = b.u32[d.term_off:d.term_off + d.terms * K_TERM_REC_F4 * 4].reshape(d.terms, K_TERM_REC_F4, 4)
    rec_f = b.f32[d.term_off:d.term_off + d.terms * K_TERM_REC_F4 * 4].reshape(d.terms, K_TERM_REC_F4, 4)
    assert len(b.terms) == d.terms
    for ti, t in enumerate(b.terms):
        lits = [o | (0 if pos else K_LITNEG) for o, pos in t]
        assert [int(v) for v in rec_u[ti, 0, :2]] == (lits + [K_NOLIT])[:2]
        kinds = 0
        for x, (o, _) in enumerate(t):
            pc = b.pc_of[o]
            nm = b.prog[pc].u0
            if 1 <= nm <= 2 and all(b.prog[pc + 1 + m].op == wl.WO_LEAF_SPHERE for m in range(nm)):
                kinds |= (1 if nm == 1 else 2) << (2 * x)
                for m in range(2):  # a single sphere repeats as member 1
                    assert list(rec_f[ti, 1 + 2 * x + m]) == list(b.prog[pc + 1 + (m if m < nm else 0)].f)[:4]
        if len(t) == 1:
            kinds |= 1 << 2  # no second literal: a dummy sphere, masked out
        assert int(rec_u[ti, 0, 2]) == kinds and rec_u[ti, 0, 3] == 0


def test_one_primitive(hostonly):
    r = wl.Renderer("one", max_nodes=16)
    r.sphere(1.0)
    b = Built(*r.program(), *r.materials())
    r.close()
    d = b.d
    assert b.nprim == 1 and b.kind_of() == 3
    assert (d.nodes, d.depth, d.top, d.always) == (0, 0, 0, 0) and d.root == K_LEAF | 0
    assert b.walk() == ([], [(0, None, None)])
    assert b.lds == 0 and len(b.blob) == d.leaf_off * 4 + 64 and list(b.kind) == [1]


def test_zero_primitives(hostonly):
    b = Built((wl.WoRec * 1)(), 0, 0, (wl.WoMaterial * 1)(), 0)
    d = b.d
    assert b.blob == b"" and b.kind_of() == 0 and d.root == K_NOREF and b.lds == 0
    assert all(getattr(d, n) == 0 for n, _ in d._fields_ if n != "root")
