// lane_bvh_build.cpp -- the host builder of the lane tracer's ordered BVH
// (wo_tracers.h, LaneTracer): from a compiled program to a descriptor and one
// packed blob (lane_bvh.h).  Plain C++: no kernels, no runtime calls, no device.
// The tree is over the primitives of a union-only program, over the terms of a
// union of small conjunctions, else over the primitives of the general tree.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <utility>
#include <vector>

#include "wo_dev.h"

using namespace wolbvh;

namespace {

struct F4 {
    float x, y, z, w;
};
static_assert(sizeof(F4) == 16, "a float4");
static_assert(sizeof(WoRec) == 32 && sizeof(WoMaterial) == 32, "leaf table entries are 2 x 32 bytes");

float bits_f(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

// Whether the program is union-only (the lane tracer's union count), and the
// ordinal -> program pc map.
bool scan_program(WoRec const* prog, uint32_t n_recs, uint32_t n_prims, std::vector<uint32_t>& ordpc) {
    bool union_only = n_prims > 0;
    ordpc.assign(n_prims ? n_prims : 1u, 0u);
    for (uint32_t pc = 0; pc < n_recs;) {
        const uint32_t op = prog[pc].op;
        if (op == WO_OP_PRIM) {
            if (prog[pc].u1 < n_prims) ordpc[prog[pc].u1] = pc;
            pc += 1u + prog[pc].u0;
        } else {
            if (op != WO_OP_UNION && op != WO_OP_BOUND) union_only = false;
            ++pc;
        }
    }
    return union_only;
}

// Axis-aligned box of a convex primitive from its members (spheres, axis-aligned
// half-spaces; general planes bound nothing), in double; false if unbounded or
// empty.
bool prim_aabb(WoRec const* prog, uint32_t pc, double lo[3], double hi[3]) {
    for (int a = 0; a < 3; ++a) {
        lo[a] = -INFINITY;
        hi[a] = INFINITY;
    }
    for (uint32_t m = 0; m < prog[pc].u0; ++m) {
        const WoRec& L = prog[pc + 1u + m];
        if (L.op == WO_LEAF_SPHERE) {
            const double r = sqrt((double)L.f[3]);
            for (int a = 0; a < 3; ++a) {
                lo[a] = fmax(lo[a], (double)L.f[a] - r);
                hi[a] = fmin(hi[a], (double)L.f[a] + r);
            }
        } else if (L.op == WO_LEAF_HALFSPACE && L.u1 >= 1u && L.u1 <= 3u) {
            const int a = (int)L.u1 - 1;  // s * x_a <= h
            if (L.f[a] > 0.0f)
                hi[a] = fmin(hi[a], (double)L.f[3]);
            else
                lo[a] = fmax(lo[a], -(double)L.f[3]);
        }
    }
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || lo[a] > hi[a]) return false;
    return true;
}

// What a box grows by on each side of an axis, so that the kernels' float slab
// tests stay conservative.
double slack(double lo, double hi) { return 1e-4 * (fabs(lo) + fabs(hi) + fabs(hi - lo)) + 1e-5; }

struct LbPrim {
    double lo[3], hi[3], c[3];
    uint32_t ord;
    void centre() {
        for (int a = 0; a < 3; ++a) c[a] = 0.5 * (lo[a] + hi[a]);
    }
    void expand() {
        for (int a = 0; a < 3; ++a) {
            const double m = slack(lo[a], hi[a]);
            lo[a] -= m;
            hi[a] += m;
        }
        centre();
    }
};

struct LbBox {
    double lo[3], hi[3];
    void empty() {
        for (int a = 0; a < 3; ++a) {
            lo[a] = INFINITY;
            hi[a] = -INFINITY;
        }
    }
    void grow(const double* l, const double* h) {
        for (int a = 0; a < 3; ++a) {
            lo[a] = fmin(lo[a], l[a]);
            hi[a] = fmax(hi[a], h[a]);
        }
    }
    double area() const {
        const double x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
        return x < 0.0 ? 0.0 : 2.0 * (x * y + y * z + z * x);
    }
};

uint32_t ceil_log2(uint32_t c) {
    uint32_t k = 0;
    while ((1ull << k) < c) ++k;
    return k;
}

// Binned-SAH build over prims[b, e) with at most `levels` internal levels below
// (ceil_log2(e - b) <= levels on entry); returns the subtree's ref and its
// depth.  A SAH split that would leave a child more primitives than its levels
// can hold becomes the median split, which always fits.  Node n is written to
// nodes[4n..4n+3] as the two children's boxes (rounded outward to float) with
// their refs in the .w of the first two.
uint32_t lb_build(std::vector<LbPrim>& prims, uint32_t b, uint32_t e, uint32_t levels, std::vector<F4>& nodes,
                  LbBox& box_out, uint32_t& depth_out) {
    box_out.empty();
    for (uint32_t i = b; i < e; ++i) box_out.grow(prims[i].lo, prims[i].hi);
    depth_out = 0;
    if (e - b == 1u) return kLeafRef | prims[b].ord;
    LbBox cb;
    cb.empty();
    for (uint32_t i = b; i < e; ++i) cb.grow(prims[i].c, prims[i].c);
    int axis = 0;
    for (int a = 1; a < 3; ++a)
        if (cb.hi[a] - cb.lo[a] > cb.hi[axis] - cb.lo[axis]) axis = a;
    uint32_t mid = b + (e - b) / 2u;
    const double ext = cb.hi[axis] - cb.lo[axis];
    if (ext > 0.0) {
        constexpr int kBins = 16;
        LbBox bb[kBins];
        uint32_t bn[kBins] = {};
        for (int k = 0; k < kBins; ++k) bb[k].empty();
        auto bin_of = [&](const LbPrim& p) {
            int k = (int)((p.c[axis] - cb.lo[axis]) / ext * kBins);
            return k < 0 ? 0 : (k >= kBins ? kBins - 1 : k);
        };
        for (uint32_t i = b; i < e; ++i) {
            const int k = bin_of(prims[i]);
            bb[k].grow(prims[i].lo, prims[i].hi);
            ++bn[k];
        }
        double best = INFINITY;
        int split = -1;
        for (int s = 1; s < kBins; ++s) {
            LbBox l, r;
            l.empty();
            r.empty();
            uint32_t nl = 0, nr = 0;
            for (int k = 0; k < s; ++k) l.grow(bb[k].lo, bb[k].hi), nl += bn[k];
            for (int k = s; k < kBins; ++k) r.grow(bb[k].lo, bb[k].hi), nr += bn[k];
            if (!nl || !nr) continue;
            const double cost = l.area() * nl + r.area() * nr;
            if (cost < best) best = cost, split = s;
        }
        if (split > 0) {
            auto it = std::partition(prims.begin() + b, prims.begin() + e,
                                     [&](const LbPrim& p) { return bin_of(p) < split; });
            mid = (uint32_t)(it - prims.begin());
        }
    }
    if (mid == b || mid == e || ceil_log2(mid - b) >= levels || ceil_log2(e - mid) >= levels) {
        // no useful split, or one too deep for the lane stack: the median along the axis
        mid = b + (e - b) / 2u;
        std::nth_element(prims.begin() + b, prims.begin() + mid, prims.begin() + e,
                         [&](const LbPrim& x, const LbPrim& y) { return x.c[axis] < y.c[axis]; });
    }
    const uint32_t n = (uint32_t)(nodes.size() / 4u);
    nodes.resize(nodes.size() + 4u);
    LbBox lb, rb;
    uint32_t ld, rd;
    const uint32_t lref = lb_build(prims, b, mid, levels - 1u, nodes, lb, ld);
    const uint32_t rref = lb_build(prims, mid, e, levels - 1u, nodes, rb, rd);
    depth_out = 1u + (ld > rd ? ld : rd);
    auto down = [](double v) { return nextafterf((float)v, -INFINITY); };
    auto up = [](double v) { return nextafterf((float)v, INFINITY); };
    F4* q = &nodes[4u * n];
    q[0] = F4{down(lb.lo[0]), down(lb.lo[1]), down(lb.lo[2]), bits_f(lref)};
    q[1] = F4{up(lb.hi[0]), up(lb.hi[1]), up(lb.hi[2]), bits_f(rref)};
    q[2] = F4{down(rb.lo[0]), down(rb.lo[1]), down(rb.lo[2]), 0.0f};
    q[3] = F4{up(rb.hi[0]), up(rb.hi[1]), up(rb.hi[2]), 0.0f};
    return n;
}

// 4-wide tree from lb_build's binary one (refs before the breadth-first order):
// a node takes its two children and, while it has fewer than four, replaces the
// internal child of largest surface area by that child's two children.  Node n
// is written to n4[7n..7n+6]: lo.x, hi.x, lo.y, hi.y, lo.z, hi.z of the four
// children (the binary nodes' expanded, outward-rounded boxes), then their refs
// (kNoRef for an empty slot; lb_bfs turns them into 16-bit refs, kNoRef16).
// `levels` = internal levels on the longest path.
struct Lb4Child {
    float lo[3], hi[3];
    uint32_t ref;
    double area() const {
        const double x = (double)hi[0] - lo[0], y = (double)hi[1] - lo[1], z = (double)hi[2] - lo[2];
        return 2.0 * (x * y + y * z + z * x);
    }
};
void lb_children2(const std::vector<F4>& n2, uint32_t n, Lb4Child out[2]) {
    const F4* q = &n2[4u * n];
    const F4 lo[2] = {q[0], q[2]}, hi[2] = {q[1], q[3]};
    for (int c = 0; c < 2; ++c) {
        out[c].lo[0] = lo[c].x, out[c].lo[1] = lo[c].y, out[c].lo[2] = lo[c].z;
        out[c].hi[0] = hi[c].x, out[c].hi[1] = hi[c].y, out[c].hi[2] = hi[c].z;
        memcpy(&out[c].ref, c == 0 ? &q[0].w : &q[1].w, sizeof(uint32_t));
    }
}
uint32_t lb_collapse4(const std::vector<F4>& n2, uint32_t n, std::vector<F4>& n4, uint32_t& levels) {
    std::vector<Lb4Child> ch(2);
    lb_children2(n2, n, ch.data());
    while (ch.size() < 4u) {
        int pick = -1;
        double best = -1.0;
        for (int i = 0; i < (int)ch.size(); ++i)
            if (!(ch[i].ref & kLeafRef) && ch[i].area() > best) best = ch[i].area(), pick = i;
        if (pick < 0) break;
        Lb4Child sub[2];
        lb_children2(n2, ch[pick].ref, sub);
        ch[pick] = sub[0];
        ch.push_back(sub[1]);
    }
    const uint32_t me = (uint32_t)(n4.size() / 7u);
    n4.resize(n4.size() + 7u);
    levels = 1u;
    uint32_t refs[4];
    for (uint32_t i = 0; i < 4u; ++i) {
        if (i >= ch.size()) {
            refs[i] = kNoRef;
        } else if (ch[i].ref & kLeafRef) {
            refs[i] = ch[i].ref;
        } else {
            uint32_t lv = 0;
            refs[i] = lb_collapse4(n2, ch[i].ref, n4, lv);
            levels = std::max(levels, 1u + lv);
        }
    }
    float v[7][4];
    for (uint32_t i = 0; i < 4u; ++i) {
        const bool has = i < ch.size();
        for (int a = 0; a < 3; ++a) {
            v[2 * a][i] = has ? ch[i].lo[a] : 0.0f;
            v[2 * a + 1][i] = has ? ch[i].hi[a] : 0.0f;
        }
        memcpy(&v[6][i], &refs[i], sizeof(float));  // full refs here; 16-bit after lb_bfs
    }
    for (int k = 0; k < 7; ++k) n4[7u * me + (uint32_t)k] = F4{v[k][0], v[k][1], v[k][2], v[k][3]};
    return me;
}

// Breadth-first node order (the root becomes 0): the top levels are then nodes
// [0, k), the ones every walk visits first, and they are staged in LDS (desc.top).
// A binary node's two refs are the .w of its first two float4; a 4-wide node's four
// are its seventh float4, and leave in their 16-bit form (the kernel's sort keys and
// stack entries; refs < 2^15 checked by the caller).
void lb_bfs(std::vector<F4>& nodes, uint32_t root, bool wide) {
    const uint32_t f4 = wide ? 7u : 4u, nref = wide ? 4u : 2u, first = wide ? 24u : 3u, stride = wide ? 1u : 4u;
    const uint32_t nn = (uint32_t)(nodes.size() / f4);
    auto ref_of = [&](std::vector<F4>& v, uint32_t n, uint32_t c) {
        return reinterpret_cast<float*>(v.data()) + (size_t)n * f4 * 4u + first + c * stride;
    };
    auto ref_at = [&](uint32_t n, uint32_t c) {
        uint32_t u;
        memcpy(&u, ref_of(nodes, n, c), sizeof u);
        return u;
    };
    std::vector<uint32_t> order, newidx(nn, 0u);
    order.push_back(root);
    for (size_t h = 0; h < order.size(); ++h)
        for (uint32_t c = 0; c < nref; ++c) {
            const uint32_t r = ref_at(order[h], c);
            if (!(r & kLeafRef)) order.push_back(r);  // (kNoRef has the leaf bit)
        }
    for (uint32_t i = 0; i < nn; ++i) newidx[order[i]] = i;
    std::vector<F4> bfs(nodes.size());
    for (uint32_t i = 0; i < nn; ++i) {
        for (uint32_t k = 0; k < f4; ++k) bfs[f4 * i + k] = nodes[f4 * order[i] + k];
        for (uint32_t c = 0; c < nref; ++c) {
            uint32_t r = ref_at(order[i], c);
            if (!(r & kLeafRef)) r = newidx[r];
            if (wide) r = r == kNoRef ? kNoRef16 : ((r & 0x7fffu) | ((r >> 16) & 0x8000u));
            memcpy(ref_of(bfs, i, c), &r, sizeof r);
        }
    }
    nodes.swap(bfs);
}

// ---- union of conjunctions (the lane tracer's term mode) ----
// A program whose root is a union of TERMS, each a conjunction of at most
// kTermLits literals (a primitive or its complement: a DIFF of one primitive by
// another is a AND NOT b) and each primitive in one term: csg256 / csg512
// balanced's pairs, csg32's box minus sphere.  Along a ray, a term's value can
// only change at an event of its own literals, so the root (a union) changes
// exactly when the count of true terms crosses 0 -- the union-only sweep with
// term transitions in place of primitive events (LaneTracer::visit_term).
// Literal encoding: ordinal | kLitNeg for a complement.

typedef std::vector<std::vector<uint32_t>> Terms;

struct TermSub {
    int kind;  // 0 conjunction (lits), 1 union of conjunctions (terms), 2 not expressible
    std::vector<uint32_t> lits;
    Terms terms;
};

// The root's terms, or false when the program is not such a union.
bool extract_terms(WoRec const* prog, uint32_t n_recs, uint32_t n_prims, Terms& terms) {
    std::vector<TermSub> st;
    auto bad = []() { TermSub t; t.kind = 2; return t; };
    auto as_terms = [](const TermSub& x) { return x.kind == 0 ? Terms{x.lits} : x.terms; };
    // NOT of a union of single positive literals (a difference's right operand)
    auto negated = [](const TermSub& x, std::vector<uint32_t>& out) {
        if (x.kind == 0) {
            if (x.lits.size() != 1u || (x.lits[0] & kLitNeg)) return false;
            out.push_back(x.lits[0] | kLitNeg);
            return true;
        }
        if (x.kind != 1) return false;
        for (const auto& t : x.terms) {
            if (t.size() != 1u || (t[0] & kLitNeg)) return false;
            out.push_back(t[0] | kLitNeg);
        }
        return true;
    };
    for (uint32_t pc = 0; pc < n_recs;) {
        const WoRec& r = prog[pc];
        if (r.op == WO_OP_PRIM) {
            TermSub t;
            t.kind = 0;
            t.lits.push_back(r.u1);
            st.push_back(t);
            pc += 1u + r.u0;
            continue;
        }
        ++pc;
        if (r.op == WO_OP_BOUND) continue;  // a culling hint: evaluators may ignore it
        if (st.size() < 2u) return false;
        TermSub b = st.back();
        st.pop_back();
        TermSub a = st.back();
        st.pop_back();
        TermSub out = bad();
        if (a.kind != 2 && b.kind != 2) {
            if (r.op == WO_OP_UNION) {
                out.kind = 1;
                out.terms = as_terms(a);
                const auto tb = as_terms(b);
                out.terms.insert(out.terms.end(), tb.begin(), tb.end());
            } else if (r.op == WO_OP_INTER && a.kind == 0 && b.kind == 0) {
                out.kind = 0;
                out.lits = a.lits;
                out.lits.insert(out.lits.end(), b.lits.begin(), b.lits.end());
            } else if ((r.op == WO_OP_DIFF || r.op == WO_OP_RDIFF)) {
                const TermSub& keep = r.op == WO_OP_DIFF ? a : b;  // DIFF: a AND NOT b; RDIFF: b AND NOT a
                const TermSub& sub = r.op == WO_OP_DIFF ? b : a;
                std::vector<uint32_t> neg;
                if (keep.kind == 0 && negated(sub, neg)) {
                    out.kind = 0;
                    out.lits = keep.lits;
                    out.lits.insert(out.lits.end(), neg.begin(), neg.end());
                }
            }
        }
        st.push_back(out);
    }
    if (st.size() != 1u || st[0].kind == 2) return false;
    // (`terms` is written only on success: the caller builds term records from whatever it holds)
    Terms got = as_terms(st[0]);
    std::vector<uint8_t> seen(n_prims, 0);
    for (const auto& t : got) {
        if (t.empty() || t.size() > kTermLits) return false;
        for (uint32_t l : t) {
            const uint32_t o = l & ~kLitNeg;
            if (o >= n_prims || seen[o]) return false;  // one term per primitive
            seen[o] = 1;
        }
    }
    terms = std::move(got);
    return true;
}

// ---- the build's stages ----

// The general tree over the primitives, BOUND records dropped: refs [0, P) are the
// primitives' leaves, [P, P + nodes) the binops.
struct GeneralTree {
    std::vector<uint32_t> gpar, gnode;  // parent per ref (kNoRef: the root); left | right << 15 | op << 30
    uint32_t root = kNoRef;
};

// 1 with the tree, 0 when it has no lane form (refs beyond 15 bits), -1 with a message
int general_tree(WoRec const* prog, uint32_t n_recs, uint32_t n_prims, GeneralTree& g, char* err, size_t errlen) {
    g.gpar.assign(n_prims, kNoRef);
    std::vector<uint32_t> st;
    for (uint32_t pc = 0; pc < n_recs;) {
        const WoRec& r = prog[pc];
        if (r.op == WO_OP_PRIM) {
            st.push_back(r.u1);
            pc += 1u + r.u0;
            continue;
        }
        ++pc;
        if (r.op == WO_OP_BOUND) continue;
        if (st.size() < 2u) {
            snprintf(err, errlen, "malformed program (binop without operands)");
            return -1;
        }
        const uint32_t b = st.back();
        st.pop_back();
        const uint32_t a = st.back();
        st.pop_back();
        const uint32_t op = r.op == WO_OP_UNION ? 0u : r.op == WO_OP_INTER ? 1u : r.op == WO_OP_DIFF ? 2u : 3u;
        const uint32_t n = n_prims + (uint32_t)g.gnode.size();
        g.gnode.push_back(a | (b << kGRefBits) | (op << 30));
        g.gpar.push_back(kNoRef);
        g.gpar[a] = n;
        g.gpar[b] = n;
        st.push_back(n);
    }
    if (st.size() != 1u || g.gpar.size() > kGRefMask) return 0;
    g.root = st[0];
    return 1;
}

// Per ordinal: the inline geometry of a single-sphere primitive.
struct PrimTables {
    std::vector<F4> geo;
    std::vector<uint32_t> kind;
};

// What the tree is built over (primitives, or terms in term mode): the bounded
// ones with their expanded boxes, and the ordinals every walk visits.
struct Leaves {
    std::vector<LbPrim> prims;
    std::vector<uint32_t> always;
};

// The primitives' tables and, with `boxes`, each primitive as a leaf.
int prim_tables(WoRec const* prog, uint32_t n_recs, uint32_t n_prims, bool boxes, PrimTables& pt, Leaves& lv, char* err,
                size_t errlen) {
    pt.geo.assign(n_prims, F4{0.0f, 0.0f, 0.0f, 0.0f});
    pt.kind.assign(n_prims, 0u);
    for (uint32_t pc = 0; pc < n_recs;) {
        const WoRec& r = prog[pc];
        if (r.op != WO_OP_PRIM) {
            ++pc;
            continue;
        }
        const uint32_t ord = r.u1;
        if (ord >= n_prims) {
            snprintf(err, errlen, "primitive ordinal out of range");
            return -1;
        }
        const WoRec& L = prog[pc + 1u];
        if (r.u0 == 1u && L.op == WO_LEAF_SPHERE) {
            pt.geo[ord] = F4{L.f[0], L.f[1], L.f[2], L.f[3]};
            pt.kind[ord] = 1u;
        }
        if (boxes) {
            LbPrim p;
            p.ord = ord;
            if (prim_aabb(prog, pc, p.lo, p.hi)) {
                p.expand();
                lv.prims.push_back(p);
            } else {
                lv.always.push_back(ord);
            }
        }
        pc += 1u + r.u0;
    }
    return 0;
}

// Term mode: each term's record (lane_bvh.h kTermRec*), and each term as a leaf.  A
// term's box is the meet of its positive literals' boxes (its value, and every
// change of it, lies inside each of them); a term with no bounded positive literal
// goes to the always list.
void term_leaves(WoRec const* prog, const Terms& terms, const std::vector<uint32_t>& pc_of, std::vector<F4>& term_recs,
                 Leaves& lv) {
    for (uint32_t ti = 0; ti < (uint32_t)terms.size(); ++ti) {
        const auto& t = terms[ti];
        // inline geometry: a literal that is one sphere, or two sphere members
        F4 rec[kTermRecF4];
        for (uint32_t k = 0; k < kTermRecF4; ++k) rec[k] = F4{0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t kinds = 0;
        for (uint32_t x = 0; x < (uint32_t)t.size(); ++x) {
            const uint32_t pc = pc_of[t[x] & ~kLitNeg];
            const uint32_t nm = prog[pc].u0;
            bool spheres = nm >= 1u && nm <= 2u;
            for (uint32_t m = 0; m < nm && spheres; ++m) spheres = prog[pc + 1u + m].op == WO_LEAF_SPHERE;
            if (!spheres) continue;
            kinds |= (nm == 1u ? kTermLitSphere : kTermLitSphere2) << (2u * x);
            for (uint32_t m = 0; m < 2u; ++m) {  // a single sphere repeats as member 1 (a no-op meet)
                const WoRec& L = prog[pc + 1u + (m < nm ? m : 0u)];
                rec[1u + 2u * x + m] = F4{L.f[0], L.f[1], L.f[2], L.f[3]};
            }
        }
        if (t.size() == 1u) kinds |= kTermLitSphere << 2u;  // no second literal: a dummy sphere, masked out
        rec[0] = F4{bits_f(t[0]), bits_f(t.size() > 1u ? t[1] : kNoLit), bits_f(kinds), 0.0f};
        term_recs.insert(term_recs.end(), rec, rec + kTermRecF4);
        LbPrim p;
        p.ord = ti;
        bool bounded = false;
        for (int a = 0; a < 3; ++a) {
            p.lo[a] = -INFINITY;
            p.hi[a] = INFINITY;
        }
        for (uint32_t l : t) {
            if (l & kLitNeg) continue;
            double lo[3], hi[3];
            if (!prim_aabb(prog, pc_of[l], lo, hi)) continue;
            bounded = true;
            for (int a = 0; a < 3; ++a) {
                p.lo[a] = fmax(p.lo[a], lo[a]);
                p.hi[a] = fmin(p.hi[a], hi[a]);
            }
        }
        if (!bounded) {
            lv.always.push_back(ti);
            continue;
        }
        for (int a = 0; a < 3; ++a)
            if (p.lo[a] > p.hi[a]) p.hi[a] = p.lo[a];  // an empty meet: a point box (never empty arithmetic)
        p.expand();
        lv.prims.push_back(p);
    }
}

// General tree: each primitive's relevance box, the meet of the bounds of the
// operands that gate it -- an intersection's other operand, a difference's
// left one for its right one -- along its path to the root (outside it the
// primitive cannot change the root).  The walk's leaf box becomes the meet of
// the primitive's box with it (twice the slack, so the clip's ends lie inside
// with room), a primitive whose meet is empty even with the slack never matters
// and leaves the walk (its bit stays 0), and an unbounded primitive with a bounded
// relevance box joins the BVH.  visit_leaf clips the primitive's interval to the
// box's span (gclip: lo with w = 1, hi; left empty when no primitive is clipped).
void general_leaves(WoRec const* prog, uint32_t n_prims, const std::vector<uint32_t>& pc_of, const GeneralTree& g,
                    std::vector<F4>& gclip, Leaves& lv) {
    typedef std::array<double, 6> Box;  // lo xyz, hi xyz
    const Box inf_box = {-INFINITY, -INFINITY, -INFINITY, INFINITY, INFINITY, INFINITY};
    auto meet = [](const Box& x, const Box& y) {
        Box m;
        for (int a = 0; a < 3; ++a) {
            m[a] = fmax(x[a], y[a]);
            m[3 + a] = fmin(x[3 + a], y[3 + a]);
        }
        return m;
    };
    auto hull = [](const Box& x, const Box& y) {
        Box h;
        for (int a = 0; a < 3; ++a) {
            h[a] = fmin(x[a], y[a]);
            h[3 + a] = fmax(x[3 + a], y[3 + a]);
        }
        return h;
    };
    auto slacked = [](Box x, double k) {
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(x[a]) || !std::isfinite(x[3 + a])) continue;
            const double m = k * slack(x[a], x[3 + a]);
            x[a] -= m;
            x[3 + a] += m;
        }
        return x;
    };
    const uint32_t nref = (uint32_t)g.gpar.size(), nnode = (uint32_t)g.gnode.size();
    std::vector<Box> bnd(nref, inf_box), con(nref, inf_box);
    for (uint32_t ord = 0; ord < n_prims; ++ord) {
        double lo[3], hi[3];
        if (prim_aabb(prog, pc_of[ord], lo, hi)) bnd[ord] = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
    }
    for (uint32_t i = 0; i < nnode; ++i) {  // operands before their node
        const uint32_t nd = g.gnode[i], a = nd & kGRefMask, b = (nd >> kGRefBits) & kGRefMask, op = nd >> 30;
        bnd[n_prims + i] = op == 0u ? hull(bnd[a], bnd[b]) : op == 1u ? meet(bnd[a], bnd[b]) : op == 2u ? bnd[a] : bnd[b];
    }
    for (uint32_t i = nnode; i-- > 0;) {  // a node before its operands
        const uint32_t nd = g.gnode[i], a = nd & kGRefMask, b = (nd >> kGRefBits) & kGRefMask, op = nd >> 30;
        const Box& c = con[n_prims + i];
        con[a] = op == 1u || op == 3u ? meet(c, bnd[b]) : c;  // b AND NOT a: a gated by b
        con[b] = op == 1u || op == 2u ? meet(c, bnd[a]) : c;  // a AND NOT b: b gated by a
    }
    gclip.assign(2u * n_prims, F4{0.0f, 0.0f, 0.0f, 0.0f});
    bool clipped = false;
    for (uint32_t ord = 0; ord < n_prims; ++ord) {
        const Box& c = con[ord];
        bool bounded = false;
        for (int a = 0; a < 6; ++a) bounded = bounded || std::isfinite(c[a]);
        if (bounded) {
            const Box cs = slacked(c, 1.0);
            auto fl = [](double v) { return (float)fmax(-1e30, fmin(1e30, v)); };
            gclip[2u * ord] = F4{fl(cs[0]), fl(cs[1]), fl(cs[2]), 1.0f};  // w != 0: clip
            gclip[2u * ord + 1u] = F4{fl(cs[3]), fl(cs[4]), fl(cs[5]), 0.0f};
            clipped = true;
        }
        const Box m = meet(slacked(bnd[ord], 2.0), slacked(c, 2.0));
        bool empty = false, finite = true;
        for (int a = 0; a < 3; ++a) {
            empty = empty || m[a] > m[3 + a];
            finite = finite && std::isfinite(m[a]) && std::isfinite(m[3 + a]);
        }
        if (empty) continue;
        if (!finite) {
            lv.always.push_back(ord);
            continue;
        }
        LbPrim p;
        p.ord = ord;
        for (int a = 0; a < 3; ++a) {
            p.lo[a] = m[a];
            p.hi[a] = m[3 + a];
        }
        p.centre();
        lv.prims.push_back(p);
    }
    if (!clipped) gclip.clear();
}

// Leaves far larger than most (diagonal over 16 medians) would bloat every box
// above them: they join the always list.
void drop_oversize(Leaves& lv) {
    std::vector<LbPrim>& prims = lv.prims;
    if (prims.empty()) return;
    std::vector<double> diag(prims.size());
    for (size_t i = 0; i < prims.size(); ++i) {
        double s = 0.0;
        for (int a = 0; a < 3; ++a) s += (prims[i].hi[a] - prims[i].lo[a]) * (prims[i].hi[a] - prims[i].lo[a]);
        diag[i] = sqrt(s);
    }
    std::vector<double> sorted = diag;
    std::nth_element(sorted.begin(), sorted.begin() + sorted.size() / 2, sorted.end());
    const double med = sorted[sorted.size() / 2];
    std::vector<LbPrim> kept;
    for (size_t i = 0; i < prims.size(); ++i) {
        if (prims.size() > 4u && diag[i] > 16.0 * med)
            lv.always.push_back(prims[i].ord);
        else
            kept.push_back(prims[i]);
    }
    prims.swap(kept);
}

// The tree over the leaves, in breadth-first order: binary, or 4-wide when `wide`
// is wanted and its refs fit 16 bits.  Sets root, depth, wide and nodes of d.
void build_tree(std::vector<LbPrim>& prims, bool want_wide, uint32_t nrefs, WoLaneBvhDesc& d, std::vector<F4>& nodes) {
    if (!prims.empty()) {
        // levels: SAH's freedom over the balanced tree's log2(n), within the stack's limit
        // (the balanced tree, levels = log2(n): RTIOW cover 12.20 ms against 11.60)
        uint32_t levels = ceil_log2((uint32_t)prims.size()) + 6u;
        if (levels > kLaneDepthMax) levels = kLaneDepthMax;
        LbBox root_box;
        d.root = lb_build(prims, 0u, (uint32_t)prims.size(), levels, nodes, root_box, d.depth);
        if (want_wide && !(d.root & kLeafRef) && nrefs < 0x8000u) {
            std::vector<F4> n4;
            uint32_t lv4 = 0;
            const uint32_t r4 = lb_collapse4(nodes, d.root, n4, lv4);
            if (n4.size() / 7u < 0x8000u) {
                nodes.swap(n4);
                d.root = r4;
                d.wide = 1u;
                d.depth = 3u * lv4;  // stack entries: at most three siblings per level
            }
        }
        if (!(d.root & kLeafRef)) {
            lb_bfs(nodes, d.root, d.wide != 0u);
            d.root = 0u;
        }
    }
    d.nodes = (uint32_t)(nodes.size() / lane_node_f4(d));
}

}  // namespace

int wolbvh::lane_bvh_build(WoRec const* prog, uint32_t n_recs, uint32_t n_prims, WoMaterial const* mats,
                           uint32_t n_mats, LaneBvhBuild* out, char* err, size_t errlen) {
    WoLaneBvhDesc& d = out->desc;
    d = WoLaneBvhDesc{};
    out->blob.clear();
    d.root = kNoRef;
    d.nprims = n_prims;
    d.union_only = scan_program(prog, n_recs, n_prims, out->ordpc) ? 1u : 0u;
    // not union-only: the BVH over the root's terms, when the root is a union of
    // small conjunctions; else over the primitives of the general tree
    Terms terms;
    GeneralTree g;
    if (!d.union_only && !extract_terms(prog, n_recs, n_prims, terms)) {
        if (!n_prims) return 0;
        const int rc = general_tree(prog, n_recs, n_prims, g, err, errlen);
        if (rc <= 0) return rc;
        d.general = 1u;
    }
    PrimTables pt;
    Leaves lv;
    std::vector<F4> term_recs, gclip;
    if (prim_tables(prog, n_recs, n_prims, d.union_only != 0u, pt, lv, err, errlen)) return -1;
    if (!terms.empty()) term_leaves(prog, terms, out->ordpc, term_recs, lv);
    if (d.general) general_leaves(prog, n_prims, out->ordpc, g, gclip, lv);
    drop_oversize(lv);
    if (ceil_log2((uint32_t)lv.prims.size()) > kLaneDepthMax) {  // > 2^24 primitives (launches allow 2^20)
        snprintf(err, errlen, "too many primitives for the lane BVH");
        return -1;
    }
    // 4-wide nodes for term mode over 256 terms (csg512_balanced, resumable walks: 50.1
    // -> 44.7 ms over the binary tree; non-resumable 82.0 -> 70.5); neutral on csg256
    // balanced's 65 terms, 16.4 / 16.5 ms; slower on csg32's 14, 8.9 -> 9.6, and on the
    // RTIOW cover's spheres, 11.7 -> 13.7
    std::vector<F4> nodes;
    build_tree(lv.prims, terms.size() > 256u, terms.empty() ? n_prims : (uint32_t)terms.size(), d, nodes);
    d.always = (uint32_t)lv.always.size();
    // 16-bit stack entries for 4-wide nodes and the general tree (its bits need the
    // LDS; binary trees otherwise: 32-bit, RTIOW cover 11.60 ms against 11.76 with
    // 16-bit entries and more top nodes)
    d.stack16 = d.wide || d.general;
    if (d.general && (d.nodes >= 0x8000u || n_prims >= 0x8000u)) {
        d.general = 0u;  // refs beyond the 16-bit stack entries: no lane form
        return 0;
    }
    d.gP = n_prims;
    d.gwords = (uint32_t)((g.gpar.size() + 31u) / 32u);
    d.groot = g.root;
    // the top nodes fill what the stacks (and the tree's bits) leave of kLanesBvhLds;
    // the kernels with camera-ray waves give the ring's LDS (LaneTracer::kCamMode)
    const size_t used = lane_bvh_lds(d), budget = kLanesBvhLds - (d.wide || d.general ? 0u : kCamRingLds);
    const uint32_t top = used < budget ? (uint32_t)((budget - used) / (lane_node_f4(d) * sizeof(F4))) : 0u;
    d.top = top < d.nodes ? top : d.nodes;
    d.spheres_only = terms.empty() && !d.general &&
                     std::all_of(pt.kind.begin(), pt.kind.end(), [](uint32_t k) { return k != 0u; });
    d.terms = (uint32_t)terms.size();

    // layout (lane_bvh.h) and pack.  Single-sphere scenes carry each ordinal's leaf
    // record and its material (2 x 32 B), so a hit's shading reads them in two
    // independent loads instead of the ordinal -> pc -> record -> material chain
    const size_t geo_off = nodes.size() * sizeof(F4);
    const size_t kind_off = geo_off + (size_t)n_prims * sizeof(F4);
    const size_t always_off = kind_off + (size_t)n_prims * sizeof(uint32_t);
    const size_t term_off = (always_off + lv.always.size() * sizeof(uint32_t) + 15u) & ~(size_t)15u;
    const size_t leaf_off = term_off + term_recs.size() * sizeof(F4);
    const size_t gpar_off = leaf_off + (d.spheres_only ? (size_t)n_prims * 2u * sizeof(WoRec) : 0u);
    const size_t gnode_off = gpar_off + g.gpar.size() * sizeof(uint32_t);
    const size_t gclip_off = (gnode_off + g.gnode.size() * sizeof(uint32_t) + 15u) & ~(size_t)15u;
    d.term_off = (uint32_t)(term_off / sizeof(uint32_t));
    d.leaf_off = d.spheres_only ? (uint32_t)(leaf_off / sizeof(uint32_t)) : 0u;
    d.gpar_off = (uint32_t)(gpar_off / sizeof(uint32_t));
    d.gnode_off = (uint32_t)(gnode_off / sizeof(uint32_t));
    d.gclip_off = gclip.empty() ? 0u : (uint32_t)(gclip_off / sizeof(uint32_t));
    std::vector<char>& blob = out->blob;
    blob.assign(gclip_off + gclip.size() * sizeof(F4), 0);
    auto put = [&](size_t off, const void* src, size_t bytes) {
        if (bytes) memcpy(blob.data() + off, src, bytes);
    };
    put(0u, nodes.data(), nodes.size() * sizeof(F4));
    put(geo_off, pt.geo.data(), (size_t)n_prims * sizeof(F4));
    put(kind_off, pt.kind.data(), (size_t)n_prims * sizeof(uint32_t));
    put(always_off, lv.always.data(), lv.always.size() * sizeof(uint32_t));
    put(term_off, term_recs.data(), term_recs.size() * sizeof(F4));
    if (d.spheres_only)
        for (uint32_t ord = 0; ord < n_prims; ++ord) {
            const WoRec& L = prog[out->ordpc[ord] + 1u];
            const size_t e = leaf_off + (size_t)ord * 2u * sizeof(WoRec);
            put(e, &L, sizeof(WoRec));
            if (L.u0 < n_mats) put(e + sizeof(WoRec), &mats[L.u0], sizeof(WoMaterial));
        }
    put(gpar_off, g.gpar.data(), g.gpar.size() * sizeof(uint32_t));
    put(gnode_off, g.gnode.data(), g.gnode.size() * sizeof(uint32_t));
    put(gclip_off, gclip.data(), gclip.size() * sizeof(F4));
    return 0;
}

extern "C" int wo_lane_bvh_build(WoRec const* prog, uint32_t n_recs, uint32_t n_prims, WoMaterial const* mats,
                                 uint32_t n_mats, WoLaneBvhDesc* desc, uint32_t info[3], void* blob, size_t cap,
                                 size_t* size, char* err, size_t errlen) {
    LaneBvhBuild b;
    if (lane_bvh_build(prog, n_recs, n_prims, mats, n_mats, &b, err, errlen)) return -1;
    *desc = b.desc;
    info[0] = (uint32_t)lane_bvh_lds(b.desc), info[1] = (uint32_t)kLanesBvhLds, info[2] = kLaneDepthMax;
    *size = b.blob.size();
    if (*size && *size <= cap) memcpy(blob, b.blob.data(), *size);
    return 0;
}
