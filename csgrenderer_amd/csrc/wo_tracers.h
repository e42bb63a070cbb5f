// wo_tracers.h -- the library kernels' two tracers for gfx950 (MI355X, CDNA4, wave64), device code
// only: InterpTracer walks the compiled postfix program (wave-uniform BOUND culling, sorted
// event window, bit-stack evaluation), LaneTracer walks the ordered BVH of lane_bvh.h one
// ray per lane.  The kernels that run them are path_kernels.h (frames) and query_kernels.h
// (rays, features, spans, mass, points); the shared device code (math, RNG, leaves, event
// window, shading, path loop) is wo_device_common.h.  Both HIP units include this header
// first, so every define that changes device code is made here, never in a host file:
// the library kernels' identity (the Makefile's KEY_SRCS) hashes these headers alone.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lane_bvh.h"
// the static kernels raise the wave priority while a hit's leaf and material loads issue
// (RTIOW cover 11.50 -> 11.47 ms in two pairs; the specialised kernel keeps 0: csg32 3.261 vs 3.266)
#ifndef WO_SHADE_PRIO
#define WO_SHADE_PRIO 1
#endif
#include "wo_device_common.h"
#include "wololo/wo_scene.h"

#pragma clang fp contract(off)

namespace {

using namespace wodev;

// 4-bit op codes of the per-wave compacted program (8 per dword).
// (2..5 are WO_OP_UNION, _INTER, _DIFF, _RDIFF unchanged)
constexpr uint32_t kCodePrim = 1, kCodeUnion = 2, kCodeConst0 = 6;

// Per-wave LDS scratch layout (dwords), computed on the host.
struct KLayout {
    uint32_t codes_words;  // packed 4-bit codes of the compacted program
    uint32_t ordpc_off;    // primitive ordinal -> program counter
    uint32_t hib_off;      // membership bits of ordinals >= 64: [word][64 lanes]
    uint32_t wave_words;   // stride between waves
};

struct ProgPtr {
    const WoRec* p;
    __device__ __forceinline__ WoRec operator[](uint32_t i) const { return p[i]; }
};

// `inv`/`have_inv`: the ray's reciprocal direction, computed on the first
// axis-aligned half-space met (wave-uniform condition).
template <bool kCount, class Prog>
__device__ __forceinline__ Ivl prim_interval(Prog prog, uint32_t pc, uint32_t count, F3 o, F3 d, F3& inv,
                                             bool& have_inv, WorkCounts& wk) {
    Ivl iv;
    for (uint32_t m = 0; m < count; ++m) {
        WoRec L = prog[pc + 1u + m];
        uint32_t kind = uni(L.op);
        WO_WK(kind == WO_LEAF_SPHERE ? WO_WORK_SPHERE_TESTS : WO_WORK_HALFSPACE_TESTS);
        if (kind == WO_LEAF_HALFSPACE && !have_inv && uni(L.u1) != 0u) {
            inv = f3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
            have_inv = true;
        }
        float la, lb;
        leaf_interval(L, kind, o, d, inv, la, lb);
        if (m == 0u)
            ivl_first(iv, la, lb);
        else
            ivl_meet(iv, la, lb, m);
    }
    return iv;
}

// Interpreter: walks the program record by record (wave-uniform pc).
template <bool kCountT>
struct InterpTracer {
    static constexpr bool kCount = kCountT;
    WorkCounts wk;
    uint64_t tmark;  // section timing (counting builds)
    ProgPtr prog;
    uint32_t nrec;
    uint32_t* codes;
    uint32_t* ordpc;
    uint32_t* hib;
    uint32_t lane;
    uint32_t ncodes;  // wave-uniform
    uint32_t nprims;  // wave-uniform, primitives surviving the cull
    uint64_t bits;    // membership of ordinals < 64

    __device__ __forceinline__ uint32_t bit(uint32_t ord) const {
        if (ord < 64u) return (uint32_t)(bits >> ord) & 1u;
        uint32_t w = (ord - 64u) >> 5;
        return (hib[w * 64u + lane] >> ((ord - 64u) & 31u)) & 1u;
    }
    __device__ __forceinline__ void toggle(uint32_t ord) {
        if (ord < 64u) {
            bits ^= 1ull << ord;
        } else {
            uint32_t w = (ord - 64u) >> 5;
            hib[w * 64u + lane] ^= 1u << ((ord - 64u) & 31u);
        }
    }
    // Root value over the compacted program, 32-deep bit stack, branch-free per
    // node: value = bit idx of the code's truth table, idx = 2A+B for binops (A
    // second, B top of stack) or the primitive's membership bit; binops pop two.
    //   PRIM 0b0010, UNION 0b1110, INTER 0b1000, DIFF 0b0100, RDIFF 0b0010, CONST0 0.
    static constexpr uint32_t kTruth =
        (0x2u << 4) | (0xEu << 8) | (0x8u << 12) | (0x4u << 16) | (0x2u << 20) | (0x0u << 24);
    __device__ __forceinline__ uint32_t eval_root() const {
        uint32_t st = 0, ord = 0;
        const uint32_t n = ncodes;
        for (uint32_t base = 0; base < n; base += 8u) {
            uint32_t word = uni(codes[base >> 3]);
            uint32_t m = n - base < 8u ? n - base : 8u;
            for (uint32_t j = 0; j < m; ++j) {
                uint32_t c = (word >> (4u * j)) & 15u;
                uint32_t tt = (kTruth >> (4u * c)) & 15u;
                bool isprim = c == kCodePrim;
                uint32_t pop = (c >= kCodeUnion && c < kCodeConst0) ? 2u : 0u;
                uint32_t idx = st & 3u;
                if (isprim) idx = bit(ord);
                uint32_t val = (tt >> idx) & 1u;
                st = ((st >> pop) << 1) | val;
                ord += isprim ? 1u : 0u;
            }
        }
        return st & 1u;
    }

    __device__ __forceinline__ WoRec hit_leaf(const Hit& h) const { return prog[ordpc[h.ord()] + 1u + h.member()]; }

    // Pass 1: walk the program, cull, intersect, collect the events after WO_T_MIN into
    // `win` (a cleared window of any size).  Leaves the compacted program, the ordinal ->
    // pc map and the membership bits at t_min behind; returns the bit stack, whose low
    // bit is the root's value at t_min.
    template <class Win>
    __device__ __forceinline__ uint32_t collect(F3 o, F3 d, Win& win, F3& inv, bool& have_inv) {
        const float tmin = WO_T_MIN;
        bits = 0;
        ncodes = 0;
        nprims = 0;
        uint32_t code_acc = 0;
        uint32_t hib_acc = 0;
        uint32_t st = 0;  // bit stack: the root value at t_min, evaluated on the way

        uint32_t pc = 0;
        while (pc < nrec) {
            WoRec rec = prog[pc];
            uint32_t op = uni(rec.op);
            uint32_t code;
            if (op == WO_OP_BOUND) {
                WO_WK(WO_WORK_BOUND_TESTS);
                bool may = bound_may_hit(rec.f[0], rec.f[1], rec.f[2], rec.f[3], rec.f[4], o, d);
                if (__ballot(may) != 0ull) {
                    ++pc;
                    continue;
                }
                code = kCodeConst0;
                st = st << 1;
                pc = uni(rec.u0);
            } else if (op == WO_OP_PRIM) {
                uint32_t count = uni(rec.u0);
                uint32_t ord = nprims;
                Ivl iv = prim_interval<kCount>(prog, pc, count, o, d, inv, have_inv, wk);
                uint32_t inside = 0;
                if (!(iv.a > iv.b)) {
                    inside = (iv.a <= tmin && iv.b > tmin) ? 1u : 0u;
                    if (iv.a > tmin) {
                        WO_WK(WO_WORK_EVENTS);
                        win.insert(event_key(iv.a, ord, 0u, iv.ma));
                    }
                    if (iv.b > tmin && iv.b < kInf) {
                        WO_WK(WO_WORK_EVENTS);
                        win.insert(event_key(iv.b, ord, 1u, iv.mb));
                    }
                }
                if (ord < 64u) {
                    bits |= (uint64_t)inside << ord;
                } else {
                    uint32_t sh = (ord - 64u) & 31u;
                    hib_acc |= inside << sh;
                    if (sh == 31u) {
                        hib[((ord - 64u) >> 5) * 64u + lane] = hib_acc;
                        hib_acc = 0;
                    }
                }
                ordpc[ord] = pc;
                nprims = ord + 1u;
                code = kCodePrim;
                st = (st << 1) | inside;
                pc += 1u + count;
            } else {
                code = op;  // WO_OP_UNION..RDIFF share values with the codes
                uint32_t tt = (kTruth >> (4u * code)) & 15u;
                st = ((st >> 2) << 1) | ((tt >> (st & 3u)) & 1u);
                ++pc;
            }
            uint32_t slot = ncodes & 7u;
            code_acc |= code << (4u * slot);
            if (slot == 7u) {
                codes[ncodes >> 3] = code_acc;
                code_acc = 0;
            }
            ++ncodes;
        }
        if (ncodes & 7u) codes[ncodes >> 3] = code_acc;
        if (nprims > 64u && ((nprims - 64u) & 31u)) hib[((nprims - 64u) >> 5) * 64u + lane] = hib_acc;
        return st;
    }

    // The window ran empty but had dropped events: re-collect the events strictly
    // after `key` (the membership state carries on).
    template <class Win>
    __device__ __forceinline__ void recollect(F3 o, F3 d, uint64_t key, Win& win, F3& inv, bool& have_inv) {
        const float tmin = WO_T_MIN;
        WO_WK(WO_WORK_RECOLLECTS);
        win.clear();
        uint32_t ordc = 0;
        uint32_t nwords = (ncodes + 7u) >> 3;
        for (uint32_t w = 0; w < nwords; ++w) {
            uint32_t word = uni(codes[w]);
            uint32_t n = ncodes - w * 8u;
            n = n < 8u ? n : 8u;
            for (uint32_t j = 0; j < n; ++j) {
                if (((word >> (4u * j)) & 15u) != kCodePrim) continue;
                uint32_t ppc = uni(ordpc[ordc]);
                uint32_t count = uni(prog[ppc].u0);
                Ivl iv = prim_interval<kCount>(prog, ppc, count, o, d, inv, have_inv, wk);
                if (!(iv.a > iv.b)) {
                    if (iv.a > tmin) {
                        uint64_t k2 = event_key(iv.a, ordc, 0u, iv.ma);
                        if (k2 > key) {
                            WO_WK(WO_WORK_EVENTS);
                            win.insert(k2);
                        }
                    }
                    if (iv.b > tmin && iv.b < kInf) {
                        uint64_t k2 = event_key(iv.b, ordc, 1u, iv.mb);
                        if (k2 > key) {
                            WO_WK(WO_WORK_EVENTS);
                            win.insert(k2);
                        }
                    }
                }
                ++ordc;
            }
        }
    }

    // Nearest change of the root's membership after WO_T_MIN along o + t d.
    __device__ __forceinline__ bool trace(F3 o, F3 d, Hit& hit) {
        Window win;
        win.clear();
        F3 inv = f3(0.0f, 0.0f, 0.0f);
        bool have_inv = false;
        const uint32_t st = collect(o, d, win, inv, have_inv);

        // pass 2: sweep events in key order; the first root flip is the hit
        if (win.empty()) return false;
        uint32_t root = st & 1u;
        while (!win.empty()) {
            uint64_t key = win.pop();
            WO_WK(WO_WORK_SWEEP_STEPS);
            uint32_t ord = key_ord(key);
            toggle(ord);
            uint32_t r = eval_root();
            if (r != root) {
                hit_from_key(key, r, hit);
                return true;
            }
            root = r;
            if (win.empty() && win.dropped()) recollect(o, d, key, win, inv, have_inv);
        }
        return false;
    }
};

// ---------------------------------------------------------------------------
// Lane traversal (scenes like the RTIOW cover: hundreds of primitives).  Each
// lane walks a hierarchy on its own, so a wave costs the LONGEST lane's walk
// instead of the UNION of its lanes' walks -- the difference that matters for
// incoherent bounce rays.  Union semantics need no tree evaluation: the root is
// inside iff the count of primitives containing the point is > 0; an entry event
// adds one, an exit removes one.  Results are the general algorithm's, bit for bit.
// ---------------------------------------------------------------------------

// Ordered BVH traversal (the common case).  The host builds a binary AABB
// hierarchy over the bounded primitives (lane_bvh_build.cpp; each node holds its two
// children's boxes, expanded outward), and an `always` list of the unbounded
// and outsized ones.  A lane walks it nearest child first with a short LDS
// stack and prunes every box whose near end lies beyond the nearest entry event
// found so far.  While the ray starts outside every primitive (none contains
// the point at t_min), the first event in key order is an entry -- an exit
// before any entry would need a primitive containing t_min -- and the root
// (a union) flips there: the hit is the smallest entry key, which does not
// depend on the visiting order, so the result is the general algorithm's bit for
// bit.  A ray that starts inside some primitive (counted on the way: boxes that
// contain the ray's start are never pruned) takes the general walk below.
// The refs, literals and term records are lane_bvh.h's.
using namespace wolbvh;
static_assert(kLaneBlock == kBlock, "the lane BVH's LDS is sized for the kernels' workgroup");
#ifndef WO_LANES_TERM2
#define WO_LANES_TERM2 1  // term visits of two spheres in all: two sphere tests (visit_leaf)
#endif
#ifndef WO_LANES_PRIO
#define WO_LANES_PRIO 1  // wave priority while a walk trip issues its node load (0: unchanged; RTIOW 11.67 -> 11.58 ms)
#endif
#ifndef WO_LANES_PRIO_LEAF
#define WO_LANES_PRIO_LEAF 1  // the same at a sphere leaf's geometry load (single-sphere walks; RTIOW 11.565 -> 11.505 ms)
#endif
#ifndef WO_LANES_PRIO_TERM
#define WO_LANES_PRIO_TERM 1  // the same at a term record's load (term mode; csg512 43.44 / 43.39 -> 43.37 / 43.28 ms, parity suite green with it)
#endif
#ifndef WO_LANES_FUSED_SPHERE
#define WO_LANES_FUSED_SPHERE 1
#endif

// component c (a compile-time constant after unrolling) of a float4
__device__ __forceinline__ float f4c(const float4& v, int c) { return c == 0 ? v.x : (c == 1 ? v.y : (c == 2 ? v.z : v.w)); }

// Slab test of a ray against an expanded AABB: [near, far] of the ray's overlap
// (conservative: the boxes carry the slack; `ri` = reciprocal direction with
// zero components replaced by +-1e30, `oi` = o * ri).
__device__ __forceinline__ float box_near(float4 lo, float4 hi, F3 ri, F3 oi, float& far_t) {
    const float ax = __builtin_fmaf(lo.x, ri.x, -oi.x), bx = __builtin_fmaf(hi.x, ri.x, -oi.x);
    const float ay = __builtin_fmaf(lo.y, ri.y, -oi.y), by = __builtin_fmaf(hi.y, ri.y, -oi.y);
    const float az = __builtin_fmaf(lo.z, ri.z, -oi.z), bz = __builtin_fmaf(hi.z, ri.z, -oi.z);
    const float n = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
    far_t = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
    return n;
}

// kMode (PathKind): 2 ordered BVH over union-only primitives, 3 the same over
// single-sphere primitives only (no generic-primitive code: fewer registers),
// 6 ordered BVH over the terms of a root that is a union of small conjunctions
// (the leaves and the always list hold terms), 7 ordered BVH over
// the primitives of a general tree (the events in key order, kGWin per walk, and
// the tree's value kept per lane and updated along the toggled leaf's path), 14 term mode over a
// 4-wide tree (four child boxes per node, half the dependent node
// loads of a walk; 16-bit stacks) with the resumable walk (trace_step, dynamic
// ray fetch).  Measured and removed: the general BOUND walk,
// 16-bit stacks for binary trees, 4-wide trees for primitives, resumable binary
// walks, a uniform grid and fp16 child boxes.
// events a general-tree walk collects (the smallest after `after`, sorted; with
// inserts beyond a full window's last filtered out -- csg360_nested 1029 ms at 4,
// 645 at 8, 503 at 16, 453 at 24, 440 at 32; 48 and 64 spill)
#ifndef WO_LANES_GWIN
#define WO_LANES_GWIN 32
#endif
constexpr int kGWin = WO_LANES_GWIN;
// a walk trip's node steps, then the leaf they reached, in one trip (LaneTracer::trip;
// the same steps per lane in the same order); 0 leaf phases: a trip is a node or a leaf
#ifndef WO_LANES_TRIP_NODES
#define WO_LANES_TRIP_NODES 2
#endif
#ifndef WO_LANES_TRIP_LEAVES
#define WO_LANES_TRIP_LEAVES 1
#endif
template <int kModeT, bool kCountT>
struct LaneTracer {
    static_assert(kModeT == 2 || kModeT == 3 || kModeT == 6 || kModeT == 7 || kModeT == 14, "lane tracer forms");
    static constexpr bool kCount = kCountT;
    static constexpr bool kDyn = kModeT == 14;
    static constexpr bool kResumable = kDyn;
    static constexpr int kMode = kModeT;
    static constexpr bool kWide = kMode == 14;
    static constexpr bool kSpheresOnly = kMode == 3;
    static constexpr bool kStack16 = kWide || kMode == 7;
    static constexpr bool kTerms = kMode == 6 || kMode == 14;
    static constexpr bool kGeneral = kMode == 7;
    static constexpr uint32_t kNodeF4 = kWide ? 7u : 4u;  // float4 per node
    // camera-ray waves (pathtrace_block): not for the resumable walk, nor for the general
    // tree (its bits fill the LDS)
    static constexpr int kCamMode = (kDyn || kGeneral) ? 0 : WO_LANES_CAM;
    static constexpr bool kFreshTail = kDyn || kGeneral;  // (TracerFreshTail)
    WorkCounts wk;
    uint64_t tmark;  // section timing (counting builds)
    const WoRec* __restrict__ prog;      // full program (generic primitives, hit leaves)
    const uint32_t* __restrict__ ordpc;  // ordinal -> program pc
    // ordered BVH (lane_bvh.h)
    const float4* __restrict__ lnodes;   // 4 float4 per node: childA lo|ref, childA hi|ref B, childB lo, childB hi
    const float4* __restrict__ lgeo;     // per ordinal: sphere centre, r^2 (single-sphere primitives)
    const uint32_t* __restrict__ lkind;  // per ordinal: 1 = single sphere, 0 = generic; then the always list
    // term mode: per term 5 float4 -- the two literals (ordinal | kLitNeg, or kNoLit)
    // and their inline kinds, then per literal up to two sphere members (kTermRec*)
    const float4* __restrict__ ltrec;
    uint32_t nalways, lroot, nprims;
    uint32_t* stk;                       // LDS stack column of this lane ([entry][lane])
    uint16_t* stk16;                     // the same with 16-bit entries (kStack16): leaf bit 15
    // LDS copy of nodes [0, ntop) (the top levels, BFS order).  Typed by address
    // space so the two node reads of query() stay an LDS and a global load: one
    // pointer to either would be a flat load, which waits on both counters.
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(3))) float4* LdsNodes;
    typedef const __attribute__((address_space(1))) float4* GlobalNodes;
#else
    typedef const float4* LdsNodes;
    typedef const float4* GlobalNodes;
#endif
    LdsNodes ltop;
    uint32_t ntop;
    // general tree (kGeneral): the tree's refs are its leaves (primitive ordinals,
    // [0, gP)) and internal nodes ([gP, ...)); per lane one bit per ref, the value of
    // that leaf / node at the current key (a column of gwords words in LDS, [w][lane])
    uint32_t* gbits;
    const uint32_t* __restrict__ gpar;   // per ref: its parent's ref, or kNoRef (the root)
    const uint32_t* __restrict__ gnode;  // per internal node: left | right << 15 | op << 30
    uint32_t gP, gwords, groot;
    uint64_t gw[kGWin];  // the walk's smallest event keys after `after`, ascending
    const float4* __restrict__ gclip;  // per primitive: relevance box (LaneBvh::gclip)
    F3 gri, goi;                       // the ray's reciprocal direction and o * ri (trace_general)

    // single-sphere scenes: per ordinal its leaf record, then its material (LaneBvh::leaves)
    const WoRec* __restrict__ lleaf;
    static constexpr bool kHitMaterial = kSpheresOnly;
    __device__ __forceinline__ WoRec hit_leaf(const Hit& h) const {
        if constexpr (kSpheresOnly)
            return lleaf[2u * h.ord()];  // one load (the record of the ordinal's only member)
        else
            return prog[ordpc[h.ord()] + 1u + h.member()];
    }
    // the leaf's material, copied next to its record: loaded beside it, not after it
    __device__ __forceinline__ WoMaterial hit_material(const Hit& h, const WoMaterial* __restrict__) const {
        return reinterpret_cast<const WoMaterial*>(lleaf)[2u * h.ord() + 1u];
    }

    // Interval of primitive `ord` (the interpreter's arithmetic, bit for bit).
    __device__ __forceinline__ Ivl prim_ivl(uint32_t ord, F3 o, F3 d, F3& inv, bool& have_inv) {
        Ivl iv;
        if (kSpheresOnly || lkind[ord] != 0u) {
            WO_WK(WO_WORK_SPHERE_TESTS);
            const float4 g = lgeo[ord];
            float b, ll, la, lb;
            sphere_bl(g.x, g.y, g.z, o, d, b, ll);
            sphere_interval_bl(b, ll, g.w, la, lb);
            ivl_first(iv, la, lb);
        } else {
            const uint32_t ppc = ordpc[ord];
            const uint32_t count = prog[ppc].u0;
            for (uint32_t m = 0; m < count; ++m) {
                WoRec L = prog[ppc + 1u + m];
                float la, lb;
                WO_WK(L.op == WO_LEAF_SPHERE ? WO_WORK_SPHERE_TESTS : WO_WORK_HALFSPACE_TESTS);
                if (L.op == WO_LEAF_SPHERE) {
                    sphere_interval(L.f[0], L.f[1], L.f[2], L.f[3], o, d, la, lb);
                } else if (L.u1 != 0u) {
                    if (!have_inv) {
                        inv = f3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
                        have_inv = true;
                    }
                    uint32_t ax = L.u1 - 1u;
                    halfspace_axis_interval(ax == 0u ? L.f[0] : (ax == 1u ? L.f[1] : L.f[2]), L.f[3], pick3(o, ax),
                                            pick3(d, ax), pick3(inv, ax), la, lb);
                } else {
                    halfspace_interval(L.f[0], L.f[1], L.f[2], L.f[3], o, d, la, lb);
                }
                if (m == 0u)
                    ivl_first(iv, la, lb);
                else
                    ivl_meet(iv, la, lb, m);
            }
        }
        return iv;
    }

    // One query's walk state (query / trace_step): the smallest event key > `after`
    // found so far, whether the count rises there (term mode), the node to visit
    // next and the lane stack's depth, the primitives (terms) holding t_min met so
    // far, and the re-query's lower box bound.
    struct QState {
        uint64_t best, after;
        uint32_t cur, sp, cnt;
        float tlo;
        bool up;
    };

    // A leaf of the walk (or of the always list): a primitive, or in
    // term mode a term.  Term mode: a term (a conjunction of one or two literals,
    // each a primitive or its complement) changes value only at an event of a
    // literal X, and then exactly when the other literal holds at that key; it
    // rises where X's literal becomes true (X's entry for a positive literal, its
    // exit for a complement).  A primitive is in one term, so one key changes one term.
    __device__ __forceinline__ void visit_leaf(uint32_t ref, uint32_t& cnt, QState& s, F3 o, F3 d, F3& inv,
                                               bool& have_inv) {
        const float tmin = WO_T_MIN;
        uint64_t& best = s.best;
        const uint64_t after = s.after;
        if constexpr (kTerms) {
            // the record's header and both literals' inline spheres: independent loads
            const float4* rec = ltrec + kTermRecF4 * ref;
#if WO_LANES_PRIO_TERM
            __builtin_amdgcn_s_setprio(WO_LANES_PRIO_TERM);
#endif
            const float4 hd = rec[0];
#if WO_LANES_PRIO_TERM
            __builtin_amdgcn_s_setprio(0);
#endif
            const uint2 tl = make_uint2(__float_as_uint(hd.x), __float_as_uint(hd.y));
            const uint32_t kinds = __float_as_uint(hd.z);
            uint64_t kin[2], kout[2];
            bool valid[2], pos[2];
            const bool one = tl.y == kNoLit;
            auto lit_keys = [&](int x, const Ivl& iv) {
                const uint32_t lit = x == 0 ? tl.x : tl.y;
                const uint32_t ord = lit & ~kLitNeg;
                pos[x] = !(lit & kLitNeg);
                valid[x] = !(iv.a > iv.b) & (iv.b > tmin) & !(x == 1 && one);
                kin[x] = iv.a > tmin ? event_key(iv.a, ord, 0u, iv.ma) : 0ull;
                kout[x] = iv.b < kInf ? event_key(iv.b, ord, 1u, iv.mb) : kEmptyKey;
            };
            // Two spheres in all (WO_LANES_TERM2): one literal of one or two sphere
            // members, or two literals of one sphere each (csg512's unions, differences
            // and intersections of pairs) -- two sphere tests instead of the four of the
            // record's general form, the same intervals and members (a single sphere's
            // repeated member is a no-op meet), when every lane of the wave has such a term
            const uint32_t k0 = kinds & 3u, k1 = (kinds >> 2) & 3u;
            const bool two = (k0 != 0u) & (one | ((k0 == kTermLitSphere) & (k1 == kTermLitSphere)));
            if (WO_LANES_TERM2 && __ballot(!two) == 0ull) {
                const bool two0 = k0 == kTermLitSphere2;  // literal 0's second member is the second sphere
                WO_WK_N(WO_WORK_SPHERE_TESTS, (two0 | !one) ? 2u : 1u);
                const float4 g0 = rec[1], g1 = rec[two0 ? 2 : 3];
                float la0, lb0, la1 = kInf, lb1 = -kInf;
                sphere_interval(g0.x, g0.y, g0.z, g0.w, o, d, la0, lb0);
                if (__ballot(two0 | !one) != 0ull) {
                    asm volatile("");
                    sphere_interval(g1.x, g1.y, g1.z, g1.w, o, d, la1, lb1);
                }
                Ivl i0, m0, i1;
                ivl_first(i0, la0, lb0);
                m0 = i0;
                ivl_meet(m0, la1, lb1, 1u);
                ivl_first(i1, la1, lb1);
                lit_keys(0, two0 ? m0 : i0);
                lit_keys(1, i1);
            } else {
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    const uint32_t lit = x == 0 ? tl.x : tl.y;
                    const uint32_t ord = lit & ~kLitNeg;
                    // an inline literal (one or two sphere members; a single sphere repeats
                    // itself as member 1, which leaves the interval and its members as
                    // they are, and a missing second literal is a dummy sphere masked out
                    // below) is branch-free: lanes at different terms stay converged
                    Ivl iv;
                    if ((kinds >> (2 * x)) & 3u) {
                        WO_WK_N(WO_WORK_SPHERE_TESTS, ((kinds >> (2 * x)) & 3u) == kTermLitSphere ? 1u : 2u);
                        const float4 g0 = rec[1 + 2 * x], g1 = rec[2 + 2 * x];
                        float la, lb;
                        sphere_interval(g0.x, g0.y, g0.z, g0.w, o, d, la, lb);
                        ivl_first(iv, la, lb);
                        sphere_interval(g1.x, g1.y, g1.z, g1.w, o, d, la, lb);
                        ivl_meet(iv, la, lb, 1u);
                    } else {
                        iv = prim_ivl(ord, o, d, inv, have_inv);
                    }
                    lit_keys(x, iv);
                }
            }
            // the literal's value just around key e of the other literal (keys are distinct)
            auto lit_at = [&](int x, uint64_t e) {
                const bool in = valid[x] & (kin[x] < e) & (e < kout[x]);
                return pos[x] ? in : !in;
            };
            const bool t0 = (pos[0] ? (valid[0] & (kin[0] == 0ull)) : !(valid[0] & (kin[0] == 0ull))) &
                            (one | (pos[1] ? (valid[1] & (kin[1] == 0ull)) : !(valid[1] & (kin[1] == 0ull))));
            if (t0) ++cnt;
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                const int y = 1 - x;
                const bool has = valid[x] & !(x == 1 && one);
                const uint64_t ei = kin[x], eo = kout[x];
                // selects, not branches (lanes at different terms stay converged)
                const bool ti = has & (ei != 0ull) & (ei > after) & (ei < best) & (one | lit_at(y, ei));
                WO_WK_N(WO_WORK_EVENTS, ti ? 1u : 0u);
                best = ti ? ei : best;
                s.up = ti ? pos[x] : s.up;
                const bool to = has & (eo != kEmptyKey) & (eo > after) & (eo < best) & (one | lit_at(y, eo));
                WO_WK_N(WO_WORK_EVENTS, to ? 1u : 0u);
                best = to ? eo : best;
                s.up = to ? !pos[x] : s.up;
            }
            return;
        }
        const uint32_t ord = ref;
#if WO_LANES_FUSED_SPHERE
        if constexpr (kSpheresOnly && !kGeneral) {
            // a sphere's interval [-b - s, -b + s] exists exactly when disc >= 0: the
            // count and the events inside the sqrt branch, no empty interval formed
            // (the specialised kernel's lone spheres; same bits as prim_ivl's form)
            WO_WK(WO_WORK_SPHERE_TESTS);
#if WO_LANES_PRIO_LEAF
            __builtin_amdgcn_s_setprio(WO_LANES_PRIO_LEAF);
#endif
            const float4 g = lgeo[ord];
#if WO_LANES_PRIO_LEAF
            __builtin_amdgcn_s_setprio(0);
#endif
            float b, ll;
            sphere_bl(g.x, g.y, g.z, o, d, b, ll);
            const float disc = g.w - ll;
            if (__ballot(sphere_need(b, disc)) != 0ull) {
                asm volatile("");
                if (!(disc < 0.0f)) {
                    const float s = sqrt_pt(disc), nb = -b, la = nb - s, lb = nb + s;
                    if ((la <= tmin) & (lb > tmin)) ++cnt;
                    const uint64_t k0 = event_key(la, ord, 0u, 0u), k1 = event_key(lb, ord, 1u, 0u);
                    if ((la > tmin) & (k0 > after)) {
                        WO_WK(WO_WORK_EVENTS);
                        best = k0 < best ? k0 : best;
                    }
                    if ((lb > tmin) & (lb < kInf) & (k1 > after)) {
                        WO_WK(WO_WORK_EVENTS);
                        best = k1 < best ? k1 : best;
                    }
                }
            }
            return;
        }
#endif
        Ivl iv = prim_ivl(ord, o, d, inv, have_inv);
        if constexpr (kGeneral) {
            // The primitive restricted to its relevance box (lane_bvh_build.cpp): outside it the
            // primitive cannot change the root (an intersection's other operand, or a
            // difference's left one, is empty there), so its interval is clipped to the
            // box's span, widened by a margin past the slab test's rounding.  An end
            // the clip moves is an event of the clipped primitive that never flips the
            // root, so the hit -- the first key where the root flips -- is unchanged.
            if (gclip != nullptr) {
                const float4 cl = gclip[2u * ord];
                if (__float_as_uint(cl.w) != 0u) {
                    float c1;
                    const float c0 = box_near(cl, gclip[2u * ord + 1u], gri, goi, c1);
                    const float m0 = __builtin_fmaf(-2e-5f, fabsf(c0), c0) - 1e-5f;
                    const float m1 = __builtin_fmaf(2e-5f, fabsf(c1), c1) + 1e-5f;
                    iv.a = fmaxf(iv.a, m0);
                    iv.b = fminf(iv.b, m1);
                }
            }
            if (!(iv.a > iv.b)) {
                // the first query sets the leaves that hold t_min (the tree's value at
                // t_min); every query keeps its kGWin smallest keys after `after`, and
                // prunes with the largest once it has them all
                if ((after == 0ull) & (iv.a <= tmin) & (iv.b > tmin)) gtoggle(ord);
                const uint64_t k0 = event_key(iv.a, ord, 0u, iv.ma), k1 = event_key(iv.b, ord, 1u, iv.mb);
                // a key at or beyond a full window's last cannot enter it
                if ((iv.a > tmin) & (k0 > after) & (k0 < gw[kGWin - 1])) {
                    WO_WK(WO_WORK_EVENTS);
                    ginsert(k0);
                }
                if ((iv.b > tmin) & (iv.b < kInf) & (k1 > after) & (k1 < gw[kGWin - 1])) {
                    WO_WK(WO_WORK_EVENTS);
                    ginsert(k1);
                }
                best = gw[kGWin - 1];
            }
            return;
        }
        if (!(iv.a > iv.b)) {
            if ((iv.a <= tmin) & (iv.b > tmin)) ++cnt;
            const uint64_t k0 = event_key(iv.a, ord, 0u, iv.ma), k1 = event_key(iv.b, ord, 1u, iv.mb);
            if ((iv.a > tmin) & (k0 > after)) {
                WO_WK(WO_WORK_EVENTS);
                best = k0 < best ? k0 : best;
            }
            if ((iv.b > tmin) & (iv.b < kInf) & (k1 > after)) {
                WO_WK(WO_WORK_EVENTS);
                best = k1 < best ? k1 : best;
            }
        }
    }

    // A query's start: the always list, then the walk from the root.  A re-query
    // (after != 0) prunes boxes that end before the last key: their events all lie
    // at or before it (the boxes' slack covers the slab test's rounding; the
    // margin below covers the key's own t).  The first query keeps every box that
    // holds the ray's start (the count at t_min).
    __device__ __forceinline__ void qbegin(QState& s, uint64_t after, F3 o, F3 d, F3& inv, bool& have_inv) {
        s.best = kEmptyKey;
        s.after = after;
        s.up = false;
        s.cnt = 0;
        for (uint32_t i = 0; i < nalways; ++i) visit_leaf(lkind[nprims + i], s.cnt, s, o, d, inv, have_inv);
        const float tafter = after == 0ull ? 0.0f : __uint_as_float((uint32_t)(after >> 32));
        s.tlo = fmaxf(__builtin_fmaf(-2e-5f, tafter, tafter) - 1e-6f, 0.0f);
        s.cur = lroot;
        s.sp = 0;
    }

    // One trip of the walk: a leaf, or a node (its children's boxes, nearest hit
    // child next, the other(s) pushed); then a pop when the walk has no next node.
    // WO_LANES_TRIP_NODES node steps and then WO_LANES_TRIP_LEAVES leaves in one trip:
    // a lane walks node -> node -> leaf in one trip instead of three, so the wave's
    // lanes, at different depths, still share most trips' node and leaf code.
    __device__ __forceinline__ void trip(QState& s, F3 o, F3 d, F3 ri, F3 oi, F3& inv, bool& have_inv) {
        WO_WK_WAVE(WO_WORK_SWEEP_TRIPS);  // lane tracer: walk trips per wave
        uint32_t cur = s.cur, sp = s.sp;
        const float tlo = s.tlo;
        auto pop = [&]() {
            if ((cur == kNoRef) & (sp != 0u)) {
                --sp;
                if constexpr (kStack16) {
                    const uint32_t e = stk16[sp * kBlock];
                    cur = (e & 0x7fffu) | ((e & 0x8000u) << 16);
                } else {
                    cur = stk[sp * kBlock];
                }
            }
        };
        // a leaf (not the walk's end) visited, then the next entry popped
        auto leaf_phase = [&]() {
            if (((cur & kLeafRef) != 0u) & (cur != kNoRef)) {
                visit_leaf(cur & ~kLeafRef, s.cnt, s, o, d, inv, have_inv);
                cur = kNoRef;
                pop();
            }
        };
        // the node step (the non-fused walk: or the leaf), then a pop when it ends a path
        auto node_phase = [&]() {
            const bool at_leaf = (cur & kLeafRef) != 0u;  // (the walk's end, kNoRef, included)
            if (!WO_LANES_TRIP_LEAVES && at_leaf) {
                visit_leaf(cur & ~kLeafRef, s.cnt, s, o, d, inv, have_inv);
                cur = kNoRef;
            } else if (kWide && !at_leaf) {
                // four children: lo.x, hi.x, lo.y, hi.y, lo.z, hi.z of each, then the refs
                WO_WK_N(WO_WORK_BOUND_TESTS, 4u);
                float4 q[7];
#if WO_LANES_PRIO
                __builtin_amdgcn_s_setprio(WO_LANES_PRIO);
#endif
                if (cur < ntop) {
                    const LdsNodes nd = ltop + 7u * cur;
#pragma unroll
                    for (int k = 0; k < 7; ++k) q[k] = nd[k];
                    asm volatile("");
                } else {
                    const GlobalNodes nd = (GlobalNodes)lnodes + 7u * cur;
#pragma unroll
                    for (int k = 0; k < 7; ++k) q[k] = nd[k];
                }
#if WO_LANES_PRIO
                __builtin_amdgcn_s_setprio(0);
#endif
                const float tb = s.best == kEmptyKey ? kInf : __uint_as_float((uint32_t)(s.best >> 32));
                // per child a sort key: the top 16 bits of max(near, 0) (monotone as an
                // unsigned integer; the order only steers the walk) | the child's 16-bit
                // ref; ~0 for a miss or an empty slot
                uint32_t kk[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float ax = __builtin_fmaf(f4c(q[0], c), ri.x, -oi.x), bx = __builtin_fmaf(f4c(q[1], c), ri.x, -oi.x);
                    const float ay = __builtin_fmaf(f4c(q[2], c), ri.y, -oi.y), by = __builtin_fmaf(f4c(q[3], c), ri.y, -oi.y);
                    const float az = __builtin_fmaf(f4c(q[4], c), ri.z, -oi.z), bz = __builtin_fmaf(f4c(q[5], c), ri.z, -oi.z);
                    const float n = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
                    const float f = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
                    const uint32_t r16 = __float_as_uint(f4c(q[6], c));
                    const float n0 = fmaxf(n, 0.0f);
                    const bool h = (f >= fmaxf(n0, tlo)) & (n <= tb) & (r16 != kNoRef16);
                    kk[c] = h ? ((__float_as_uint(n0) & 0xffff0000u) | r16) : 0xffffffffu;
                }
                // nearest first: a 4-key sorting network (misses sort last)
                auto ce = [&](int i, int j) {
                    const uint32_t lo = kk[i] < kk[j] ? kk[i] : kk[j], hi = kk[i] < kk[j] ? kk[j] : kk[i];
                    kk[i] = lo;
                    kk[j] = hi;
                };
                ce(0, 1);
                ce(2, 3);
                ce(0, 2);
                ce(1, 3);
                ce(1, 2);
                cur = kk[0] == 0xffffffffu ? kNoRef : (kk[0] & 0x7fffu) | ((kk[0] & 0x8000u) << 16);
                // the farther ones on the stack, farthest deepest (sp < 3 x the tree's levels)
#pragma unroll
                for (int c = 3; c >= 1; --c) {
                    if (kk[c] != 0xffffffffu) {
                        stk16[sp * kBlock] = (uint16_t)kk[c];
                        ++sp;
                    }
                }
            } else if (!kWide && !at_leaf) {
                WO_WK_N(WO_WORK_BOUND_TESTS, 2u);
                float na, nb, fa, fb;
                uint32_t ra, rb;
                {
                    float4 a0, a1, b0, b1;
#if WO_LANES_PRIO
                    __builtin_amdgcn_s_setprio(WO_LANES_PRIO);  // a wave about to issue its node load goes first
#endif
                    if (cur < ntop) {  // the top levels: LDS latency instead of a cache round trip
                        const LdsNodes nd = ltop + 4u * cur;
                        a0 = nd[0], a1 = nd[1], b0 = nd[2], b1 = nd[3];
                        asm volatile("");  // the branches' tails differ: the loads are not merged into flat loads
                    } else {
                        const GlobalNodes nd = (GlobalNodes)lnodes + 4u * cur;
                        a0 = nd[0], a1 = nd[1], b0 = nd[2], b1 = nd[3];
                    }
#if WO_LANES_PRIO
                    __builtin_amdgcn_s_setprio(0);
#endif
                    na = box_near(a0, a1, ri, oi, fa);
                    nb = box_near(b0, b1, ri, oi, fb);
                    ra = __float_as_uint(a0.w);
                    rb = __float_as_uint(a1.w);
                }
                // useful range: up to the best event so far
                const float tb = s.best == kEmptyKey ? kInf : __uint_as_float((uint32_t)(s.best >> 32));
                const bool ha = (fa >= fmaxf(na, tlo)) & (na <= tb);
                const bool hb = (fb >= fmaxf(nb, tlo)) & (nb <= tb);
                if (ha & hb) {
                    const bool a_first = na <= nb;
                    cur = a_first ? ra : rb;
                    const uint32_t other = a_first ? rb : ra;
                    if constexpr (kStack16)  // refs < 2^15 (the builder's check): the leaf flag moves to bit 15
                        stk16[sp * kBlock] = (uint16_t)((other & 0x7fffu) | ((other >> 16) & 0x8000u));
                    else
                        stk[sp * kBlock] = other;  // sp < the tree's depth (kLaneDepthMax)
                    ++sp;
                } else {
                    cur = ha ? ra : (hb ? rb : kNoRef);
                }
            }
            pop();
        };
        // (a lane at a leaf or at the walk's end skips a node step)
#pragma unroll
        for (int k = 0; k < WO_LANES_TRIP_NODES; ++k) node_phase();
#pragma unroll
        for (int k = 0; k < WO_LANES_TRIP_LEAVES; ++k) leaf_phase();
        s.cur = cur;
        s.sp = sp;
    }

    // The smallest event key > `after` (entries and exits after t_min), or
    // kEmptyKey; `inside` (first query only) counts the primitives whose
    // interval holds t_min.  Boxes are pruned beyond the best event so far; the
    // boxes holding the ray's start never are, so the count is complete.
    // `up`: the count of true members (primitives; terms in term mode) rises at
    // the returned key.
    __device__ __forceinline__ uint64_t query(F3 o, F3 d, F3 ri, F3 oi, uint64_t after, uint32_t& inside, bool& up,
                                              F3& inv, bool& have_inv) {
        QState s;
        qbegin(s, after, o, d, inv, have_inv);
        while (s.cur != kNoRef) trip(s, o, d, ri, oi, inv, have_inv);
        inside = s.cnt;
        if constexpr (kTerms)
            up = s.up;
        else  // a primitive's count rises at its entry
            up = !(s.best & kKeyTypeBit);
        return s.best;
    }

    // Events in key order, one query each, from the count of primitives holding
    // t_min; the root (count > 0) flips at the hit.  A ray that starts outside
    // every primitive needs one query: its first event is an entry.
    __device__ __forceinline__ bool trace_ordered(F3 o, F3 d, Hit& hit) {
        // culling arithmetic only: approximate reciprocals are fine (the boxes carry the slack)
        const float dx = fabsf(d.x) < 1e-30f ? copysignf(1e-30f, d.x) : d.x;
        const float dy = fabsf(d.y) < 1e-30f ? copysignf(1e-30f, d.y) : d.y;
        const float dz = fabsf(d.z) < 1e-30f ? copysignf(1e-30f, d.z) : d.z;
        const F3 ri = f3(__builtin_amdgcn_rcpf(dx), __builtin_amdgcn_rcpf(dy), __builtin_amdgcn_rcpf(dz));
        const F3 oi = f3(o.x * ri.x, o.y * ri.y, o.z * ri.z);
        F3 inv = f3(0.0f, 0.0f, 0.0f);
        bool have_inv = false;
        uint32_t cnt = 0, unused = 0;
        bool up = false;
        uint64_t key = query(o, d, ri, oi, 0ull, cnt, up, inv, have_inv);
        const uint32_t root = cnt > 0u ? 1u : 0u;
        while (key != kEmptyKey) {
            WO_WK(WO_WORK_SWEEP_STEPS);
            cnt = up ? cnt + 1u : cnt - 1u;
            const uint32_t rv = cnt > 0u ? 1u : 0u;
            if (rv != root) {
                hit_from_key(key, rv, hit);
                return true;
            }
            WO_WK(WO_WORK_RECOLLECTS);
            key = query(o, d, ri, oi, key, unused, up, inv, have_inv);
        }
        return false;
    }

    // Resumable trace (kDyn, pathtrace_block's dynamic ray fetch): the walk of a
    // query carries over between calls in `dq`, so a wave whose lanes' walks end
    // at different trips need not run its slowest lane's walk to the end before
    // the finished lanes shade and take their next rays.  Once at most
    // WO_LANES_DYN_WALKERS lanes are still walking (and `may_bail`: the tile's
    // queue still has jobs, so the finished lanes have work to fetch), the walking
    // lanes return kTracePending after a trip and resume from the same state at
    // the next call.  Each call makes at least one trip, so every walk finishes.
    // Same queries, same keys: the hit is trace_ordered's bit for bit.
    QState dq;
    uint32_t dyn_walkers;  // bail-out threshold (LaneBvh::dyn_walkers, wave-uniform)
    uint32_t dcnt;   // the count of true members at the last key processed
    bool droot;      // the root's value at t_min
    bool dfirst;     // the walk in dq is the ray's first query
    bool dpending;   // a walk is in dq (set up by an earlier call)
    __device__ __forceinline__ int trace_step(F3 o, F3 d, Hit& hit, bool may_bail) {
        const float dx = fabsf(d.x) < 1e-30f ? copysignf(1e-30f, d.x) : d.x;
        const float dy = fabsf(d.y) < 1e-30f ? copysignf(1e-30f, d.y) : d.y;
        const float dz = fabsf(d.z) < 1e-30f ? copysignf(1e-30f, d.z) : d.z;
        const F3 ri = f3(__builtin_amdgcn_rcpf(dx), __builtin_amdgcn_rcpf(dy), __builtin_amdgcn_rcpf(dz));
        const F3 oi = f3(o.x * ri.x, o.y * ri.y, o.z * ri.z);
        // the exact reciprocal (generic primitives' axis half-spaces) on first need
        // in this call: the same values whenever it is recomputed
        F3 inv = f3(0.0f, 0.0f, 0.0f);
        bool have_inv = false;
        if (!dpending) {
            qbegin(dq, 0ull, o, d, inv, have_inv);
            dfirst = true;
        }
        for (;;) {
            bool walked = false;
            while (dq.cur != kNoRef) {
                if (walked && may_bail && (uint32_t)__popcll(__ballot(true)) <= dyn_walkers) {
                    dpending = true;
                    return kTracePending;
                }
                trip(dq, o, d, ri, oi, inv, have_inv);
                walked = true;
            }
            const uint64_t key = dq.best;
            const bool up = kTerms ? dq.up : !(key & kKeyTypeBit);
            if (dfirst) {
                dcnt = dq.cnt;
                droot = dcnt > 0u;
                dfirst = false;
            }
            if (key == kEmptyKey) {
                dpending = false;
                return kTraceMiss;
            }
            WO_WK(WO_WORK_SWEEP_STEPS);
            dcnt = up ? dcnt + 1u : dcnt - 1u;
            const bool rv = dcnt > 0u;
            if (rv != droot) {
                hit_from_key(key, rv ? 1u : 0u, hit);
                dpending = false;
                return kTraceHit;
            }
            WO_WK(WO_WORK_RECOLLECTS);
            qbegin(dq, key, o, d, inv, have_inv);
        }
    }

    // ---- general tree (kGeneral) ----
    __device__ __forceinline__ uint32_t gbit(uint32_t ref) const { return (gbits[(ref >> 5) * kBlock] >> (ref & 31u)) & 1u; }
    __device__ __forceinline__ void gflip(uint32_t ref) { gbits[(ref >> 5) * kBlock] ^= 1u << (ref & 31u); }
    // toggle leaf `ord` and re-evaluate its ancestors while their values change
    __device__ __forceinline__ void gtoggle(uint32_t ord) {
        WO_WK(WO_WORK_SWEEP_STEPS);
        uint32_t ref = ord;
        gflip(ref);
        for (;;) {
            const uint32_t par = gpar[ref];
            if (par == kNoRef) break;  // ref is the root
            const uint32_t nd = gnode[par - gP];
            const uint32_t a = gbit(nd & kGRefMask), b = gbit((nd >> kGRefBits) & kGRefMask), op = nd >> 30;
            const uint32_t v = op == 0u ? (a | b) : op == 1u ? (a & b) : op == 2u ? (a & (b ^ 1u)) : (b & (a ^ 1u));
            if (v == gbit(par)) break;
            gflip(par);
            ref = par;
        }
    }
    // the sorted window's insert (branch-free: an early exit once no lane shifts
    // measured slower, 488 against 440 ms on csg360_nested)
    __device__ __forceinline__ void ginsert(uint64_t key) {
#pragma unroll
        for (int i = kGWin - 1; i > 0; --i) gw[i] = key < gw[i - 1] ? gw[i - 1] : (key < gw[i] ? key : gw[i]);
        gw[0] = key < gw[0] ? key : gw[0];
    }
    // Events in key order, kGWin per walk (the walk prunes boxes beyond the largest
    // once it holds kGWin), each toggling its primitive's leaf; the hit is the first
    // key at which the root's value differs from its value at t_min -- the general
    // sweep's hit bit for bit (the tree's value after a key is the program's value of
    // the leaves' membership there).
    __device__ __forceinline__ bool trace_general(F3 o, F3 d, Hit& hit) {
        const float dx = fabsf(d.x) < 1e-30f ? copysignf(1e-30f, d.x) : d.x;
        const float dy = fabsf(d.y) < 1e-30f ? copysignf(1e-30f, d.y) : d.y;
        const float dz = fabsf(d.z) < 1e-30f ? copysignf(1e-30f, d.z) : d.z;
        const F3 ri = f3(__builtin_amdgcn_rcpf(dx), __builtin_amdgcn_rcpf(dy), __builtin_amdgcn_rcpf(dz));
        const F3 oi = f3(o.x * ri.x, o.y * ri.y, o.z * ri.z);
        gri = ri;
        goi = oi;
        F3 inv = f3(0.0f, 0.0f, 0.0f);
        bool have_inv = false;
        for (uint32_t w = 0; w < gwords; ++w) gbits[w * kBlock] = 0u;  // every leaf and node 0
        uint64_t after = 0ull;
        uint32_t root0 = 0u;
        for (;;) {
#pragma unroll
            for (int i = 0; i < kGWin; ++i) gw[i] = kEmptyKey;
            QState s;
            qbegin(s, after, o, d, inv, have_inv);
            while (s.cur != kNoRef) trip(s, o, d, ri, oi, inv, have_inv);
            if (after == 0ull) root0 = gbit(groot);
#pragma unroll
            for (int i = 0; i < kGWin; ++i) {
                const uint64_t key = gw[i];
                if (key == kEmptyKey) return false;  // every event after `after` processed
                gtoggle(key_ord(key));
                const uint32_t rv = gbit(groot);
                if (rv != root0) {
                    hit_from_key(key, rv, hit);
                    return true;
                }
            }
            WO_WK(WO_WORK_RECOLLECTS);
            after = gw[kGWin - 1];
        }
    }

    __device__ __forceinline__ bool trace(F3 o, F3 d, Hit& hit) {
        if constexpr (kGeneral)
            return trace_general(o, d, hit);
        else
            return trace_ordered(o, d, hit);
    }
};

#ifndef WO_LANES_MIN_WAVES
#define WO_LANES_MIN_WAVES 8  // rtiow_cover: 40.0 ms at 6, 37.4 at 7, 36.5 at 8 (64 VGPRs)
#endif
#ifndef WO_LANES_BVH_MIN_WAVES
#define WO_LANES_BVH_MIN_WAVES 7  // rtiow_cover: 16.86 ms at 8, 16.63 at 7, 17.26 at 6
#endif
// The ordered-BVH tables (the sections of lane_bvh.h's blob, on the device).
struct LaneBvh {
    const float4* nodes;
    const float4* geo;
    const uint32_t* kind;  // per ordinal, then the always list
    const float4* trec;    // term mode: kTermRecF4 float4 per term
    const WoRec* leaves;   // single-sphere scenes: per ordinal its leaf record
    uint32_t nalways, root, nprims;
    uint32_t depth;        // internal levels of the tree: the lane stack's entries
    uint32_t ntop;         // nodes [0, ntop) staged in LDS after the lane stacks
    uint32_t dyn_walkers;  // resumable walk: walking lanes at which a wave bails out
    // general tree (kind 7): parent per ref, node records, leaves, words per lane, root ref
    const uint32_t* gpar;
    const uint32_t* gnode;
    const float4* gclip;  // per primitive: relevance box lo (w: 1 = clip) and hi; nullptr: none
    uint32_t gP, gwords, groot;
};

// The interpreter kernels' prologue.  stage_program: the program copied into the dynamic LDS
// by the whole workgroup (kProgInLds; a barrier follows the copy) or read where it is;
// returns the LDS behind it.  interp_setup: that, then the tracer pointed at its wave's
// scratch (KLayout) behind the program.
template <bool kProgInLds>
__device__ __forceinline__ uint32_t* stage_program(ProgPtr& prog, uint32_t* smem, const WoRec* __restrict__ gprog,
                                                   uint32_t nrec, uint32_t tid) {
    if constexpr (kProgInLds) {
        const uint4* src = reinterpret_cast<const uint4*>(gprog);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        for (uint32_t i = tid; i < nrec * 2u; i += kBlock) dst[i] = src[i];
        __syncthreads();
        prog.p = reinterpret_cast<const WoRec*>(smem);
        return smem + nrec * 8u;
    } else {
        prog.p = gprog;
        return smem;
    }
}
template <bool kProgInLds, class Tracer>
__device__ __forceinline__ void interp_setup(Tracer& tr, uint32_t* smem, const WoRec* __restrict__ gprog, uint32_t nrec,
                                             const KLayout& lay, uint32_t tid, uint32_t lane, uint32_t wave) {
    uint32_t* ws = stage_program<kProgInLds>(tr.prog, smem, gprog, nrec, tid) + wave * lay.wave_words;
    tr.nrec = nrec;
    tr.codes = ws;
    tr.ordpc = ws + lay.ordpc_off;
    tr.hib = ws + lay.hib_off;
    tr.lane = lane;
}

// The lane kernels' prologue, WO_LANE_SETUP(tr, prog, ordpc, bvh, smem), over plain names: the tracer pointed at the
// scene's tables and its lane's stack column in the dynamic LDS (lane_bvh_lds sizes it: the
// stacks, 32-bit or kStack16, then the top nodes, then a general tree's bits), and the top
// levels of the BVH copied next to the stacks by the whole workgroup.  The caller's barrier
// orders the copy before any walk.  A macro, not a function: a function takes the kernel's
// LaneBvh argument by address, which keeps the compiler's first scalar-replacement pass
// (it runs before inlining) off it, and the frame kernels' code then differs from what it
// was by spill-slot numbers and, for the general tree, by s_nop counts (tried with the
// tables by reference and by value, with and without restrict); expanded in the kernel
// the frame kernels are instruction for instruction what they were (tools/lib_isa_diff.py,
// profiles/kernel_layout_isa.txt).
#define WO_LANE_SETUP(tr, prog_, ordpc_, bvh, smem)                                                                   \
    {                                                                                                                 \
        typedef decltype(tr) Tracer_;                                                                                 \
        tr.prog = (prog_);                                                                                            \
        tr.ordpc = (ordpc_);                                                                                          \
        tr.lnodes = bvh.nodes;                                                                                        \
        tr.lgeo = bvh.geo;                                                                                            \
        tr.lkind = bvh.kind;                                                                                          \
        tr.ltrec = bvh.trec;                                                                                          \
        tr.lleaf = bvh.leaves;                                                                                        \
        tr.nalways = bvh.nalways;                                                                                     \
        tr.lroot = bvh.root;                                                                                          \
        tr.nprims = bvh.nprims;                                                                                       \
        tr.stk = (smem) + threadIdx.x;                                                                                \
        tr.stk16 = reinterpret_cast<uint16_t*>(smem) + threadIdx.x;                                                   \
        tr.ntop = 0;                                                                                                  \
        tr.ltop = (typename Tracer_::LdsNodes)nullptr;                                                                \
        if constexpr (Tracer_::kDyn) {                                                                                \
            tr.dpending = false;                                                                                      \
            tr.dyn_walkers = bvh.dyn_walkers;                                                                         \
        }                                                                                                             \
        const uint32_t stack_words_ = Tracer_::kStack16 ? (bvh.depth * kBlock + 1u) / 2u : bvh.depth * kBlock;        \
        float4* top_ = reinterpret_cast<float4*>((smem) + ((stack_words_ + 3u) & ~3u));                               \
        for (uint32_t i_ = threadIdx.x; i_ < Tracer_::kNodeF4 * bvh.ntop; i_ += kBlock) top_[i_] = bvh.nodes[i_];     \
        tr.ltop = (typename Tracer_::LdsNodes)top_;                                                                   \
        tr.ntop = bvh.ntop;                                                                                           \
        if constexpr (Tracer_::kGeneral) { /* the tree's bits after the top nodes, [word][lane] */                    \
            tr.gbits = reinterpret_cast<uint32_t*>(top_ + Tracer_::kNodeF4 * bvh.ntop) + threadIdx.x;                 \
            tr.gpar = bvh.gpar;                                                                                       \
            tr.gnode = bvh.gnode;                                                                                     \
            tr.gclip = bvh.gclip;                                                                                     \
            tr.gP = bvh.gP;                                                                                           \
            tr.gwords = bvh.gwords;                                                                                   \
            tr.groot = bvh.groot;                                                                                     \
        }                                                                                                             \
    }

// A wave's item of 64 cells of a width x rows grid (a rank's local pixels, a mass grid's
// cells): an 8 x 8 tile (lane = 8 row + column) or a 64 x 1 strip of one row, numbered
// row-major and dealt to the waves by the kernels' grid-stride loops; lane 0 of an item is
// always a cell of the grid.  Both footprints were measured; no result
// depends on them.  The host counts a launch's items with the same constructor.
template <bool kTile>
struct WaveItems {
    uint32_t across;
    uint64_t count;
    __host__ __device__ __forceinline__ WaveItems(uint32_t width, uint32_t rows) {
        across = kTile ? (width + 7u) >> 3 : (width + 63u) >> 6;
        count = (uint64_t)across * (kTile ? (rows + 7u) >> 3 : rows);
    }
    __device__ __forceinline__ void cell(uint64_t item, uint32_t lane, uint32_t& x, uint32_t& row) const {
        const uint32_t iy = (uint32_t)(item / across), ix = (uint32_t)(item - (uint64_t)iy * across);
        x = ix * (kTile ? 8u : 64u) + (kTile ? (lane & 7u) : lane);
        row = iy * (kTile ? 8u : 1u) + (kTile ? (lane >> 3) : 0u);
    }
};

}  // namespace
