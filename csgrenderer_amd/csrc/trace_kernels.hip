// trace_kernels.hip -- the per-pixel hot path of the wololo renderer for gfx950
// (MI355X, CDNA4, wave64).  Replaces the reference's fragment stage
// (src/wololo/renderer/ubershader1.frag:19-163, one invocation per pixel,
// launched by draw_frame_with_renderer, renderer.c:2085-2219).
//
// Kernels
//   ubershader_kernel  the reference shader restated bit-for-bit in IEEE fp32
//                      (sin hoisted to the host).  HBM-store bound, 16 B/pixel.
//   pathtrace_kernel   CSG path tracer, INTERPRETER form: walks the compiled
//                      postfix program (staged in LDS when it fits), wave-uniform
//                      BOUND culling, sorted event window, bit-stack evaluation.
//   wo_jit_pathtrace   the same path tracer SPECIALISED per scene: source from
//                      scene_jit.c, compiled and cached by jit_code.cpp, loaded here.
//   assemble_kernel    un-interleaves row-cyclic rank tiles after the gather.
// The shared device code (math, RNG, leaves, event window, shading, path loop)
// is wo_device_common.h; both forms agree bit-for-bit with oracle/oracle.c.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <string>
#include <vector>

#include "jit_code.h"
#include "wo_dev.h"
// the static kernels raise the wave priority while a hit's leaf and material loads issue
// (RTIOW cover 11.50 -> 11.47 ms in two pairs; the specialised kernel keeps 0: csg32 3.261 vs 3.266)
#ifndef WO_SHADE_PRIO
#define WO_SHADE_PRIO 1
#endif
#include "wo_device_common.h"
#include "wololo/wo_scene.h"

#include "static_key.inc"  // WO_STATIC_SRC_SHA: the library kernels' source identity

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

// Dynamic LDS: the BVH walk's lane stacks ([depth][kBlock] u32 or u16) and top nodes.
#ifndef WO_LANES_BVH_MIN_WAVES
#define WO_LANES_BVH_MIN_WAVES 7  // rtiow_cover: 16.86 ms at 8, 16.63 at 7, 17.26 at 6
#endif
template <int kMode, bool kCount>
#ifndef WO_LANES_TERMS_MIN_WAVES
#define WO_LANES_TERMS_MIN_WAVES 7  // csg512_balanced: 80.8 ms at 7 (13 VGPRs spilled), 82.0 at 6 (none)
#endif
#ifndef WO_LANES_DYN_MIN_WAVES
#define WO_LANES_DYN_MIN_WAVES 7
#endif
#ifndef WO_LANES_DYN_TERMS_MIN_WAVES
#define WO_LANES_DYN_TERMS_MIN_WAVES 6  // csg512_balanced: 56.4 ms at 6 (no spill), 57.2 at 7 (31 VGPRs spilled)
#endif
#ifndef WO_LANES_GENERAL_MIN_WAVES
#define WO_LANES_GENERAL_MIN_WAVES 4  // the tree's bits take ~20 KB of LDS per workgroup (csg360_nested)
#endif
__global__ __launch_bounds__(kBlock, kMode == 14  ? WO_LANES_DYN_TERMS_MIN_WAVES
                                    : kMode == 7 ? WO_LANES_GENERAL_MIN_WAVES
                                    : kMode == 6 ? WO_LANES_TERMS_MIN_WAVES
                                    : kMode == 2 ? WO_LANES_BVH_MIN_WAVES
                                                 : WO_LANES_MIN_WAVES) void pathtrace_lanes_kernel(
    const WoRec* __restrict__ prog, const uint32_t* __restrict__ ordpc, const WoMaterial* __restrict__ mats, WoFrame fr,
    uint32_t local_rows, float4* __restrict__ out, unsigned long long* __restrict__ seg_slots, PathLaunch tg,
    LaneBvh bvh) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    LaneTracer<kMode, kCount> tr;
    tr.prog = prog;
    tr.ordpc = ordpc;
    tr.lnodes = bvh.nodes;
    tr.lgeo = bvh.geo;
    tr.lkind = bvh.kind;
    tr.ltrec = bvh.trec;
    tr.lleaf = bvh.leaves;
    tr.nalways = bvh.nalways;
    tr.lroot = bvh.root;
    tr.nprims = bvh.nprims;
    tr.stk = smem + threadIdx.x;
    tr.stk16 = reinterpret_cast<uint16_t*>(smem) + threadIdx.x;
    tr.ntop = 0;
    tr.ltop = (typename LaneTracer<kMode, kCount>::LdsNodes)nullptr;
    if constexpr (LaneTracer<kMode, kCount>::kDyn) {
        tr.dpending = false;
        tr.dyn_walkers = bvh.dyn_walkers;
    }
    {
        // the top levels of the BVH next to the stacks; pathtrace_block's first
        // barrier orders the copy before any walk
        constexpr bool kStack16 = LaneTracer<kMode, kCount>::kStack16;
        const uint32_t stack_words = kStack16 ? (bvh.depth * kBlock + 1u) / 2u : bvh.depth * kBlock;
        float4* top = reinterpret_cast<float4*>(smem + ((stack_words + 3u) & ~3u));
        constexpr uint32_t kNodeF4 = LaneTracer<kMode, kCount>::kNodeF4;
        for (uint32_t i = threadIdx.x; i < kNodeF4 * bvh.ntop; i += kBlock) top[i] = bvh.nodes[i];
        tr.ltop = (typename LaneTracer<kMode, kCount>::LdsNodes)top;
        tr.ntop = bvh.ntop;
        if constexpr (LaneTracer<kMode, kCount>::kGeneral) {
            // the tree's bits after the top nodes, [word][lane]
            tr.gbits = reinterpret_cast<uint32_t*>(top + kNodeF4 * bvh.ntop) + threadIdx.x;
            tr.gpar = bvh.gpar;
            tr.gnode = bvh.gnode;
            tr.gclip = bvh.gclip;
            tr.gP = bvh.gP;
            tr.gwords = bvh.gwords;
            tr.groot = bvh.groot;
        }
    }
    pathtrace_block(tr, mats, fr, local_rows, out, seg_slots, tg);
}

// ---------------------------------------------------------------------------
// ubershader1.frag restated (ref ubershader1.frag:19-163).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void ubershader_kernel(WoFrame fr, uint32_t local_rows, float4* __restrict__ out) {
    uint32_t lx = blockIdx.x * kBlock + threadIdx.x;
    uint32_t lrow = blockIdx.y;
    if (lx >= fr.width || lrow >= local_rows) return;
    uint32_t y = local_to_global_row(fr, lrow);
    if (y >= fr.height) return;

    float resx = (float)fr.width, resy = (float)fr.height;
    float aspect = resx / resy;   // frag:20
    float fx = (float)lx + 0.5f;  // gl_FragCoord at the pixel centre,
    float fy = (float)y + 0.5f;   // OriginUpperLeft (row 0 = top)
    float stx = fx / resx;        // frag:26-29
    float sty = 1.0f - fy / resy;
    float4 res;
    if (fr.mode == WO_MODE_DEBUG_ST) {  // frag:133-138
        res = make_float4(stx, sty, 0.0f, 1.0f);
    } else {
        // camera (frag:50-60): llc = (-aspect/2, -0.5, -1); ray dir (frag:74-82), not normalised
        float dx = (0.0f - aspect * 0.5f) + stx * aspect;
        float dy = -0.5f + sty;
        float dz = -1.0f;
        // hit_sphere (frag:84-95), centre (0, 2 sin(w t), -11), r = 0.5 (frag:100-105)
        float sy = fr.sphere_y;
        float ocy = 0.0f - sy;
        float ocz = 11.0f;
        float a = (dx * dx + dy * dy) + dz * dz;
        float b = 2.0f * ((0.0f * dx + ocy * dy) + ocz * dz);
        float c = ((0.0f * 0.0f + ocy * ocy) + ocz * ocz) - 0.5f * 0.5f;
        float disc = b * b - (4.0f * a) * c;
        float t = -1.0f;
        if (!(disc < 0.0f)) t = (-b - sqrtf(disc)) / (2.0f * a);
        if (t > 0.0f) {  // frag:107-111
            float nx = dx * t - 0.0f, ny = dy * t - sy, nz = dz * t - (-11.0f);
            float len = sqrtf((nx * nx + ny * ny) + nz * nz);
            nx = nx / len;
            ny = ny / len;
            nz = nz / len;
            res = make_float4(0.5f * (nx + 1.0f), 0.5f * (ny + 1.0f), 0.5f * (nz + 1.0f), 1.0f);
        } else {  // frag:116-122
            float len = sqrtf((dx * dx + dy * dy) + dz * dz);
            float uy = dy / len;
            float s = 1.0f - uy;
            res = make_float4(s + uy * 0.5f, s + uy * 0.7f, s + uy * 1.0f, 1.0f);
        }
    }
    out[(size_t)lrow * fr.width + lx] = res;
}

template <bool kProgInLds, bool kCount>
__global__ __launch_bounds__(kBlock) void pathtrace_kernel(const WoRec* __restrict__ gprog,
                                                           const WoMaterial* __restrict__ mats, WoFrame fr,
                                                           KLayout lay, uint32_t local_rows,
                                                           float4* __restrict__ out,
                                                           unsigned long long* __restrict__ seg_slots,
                                                           PathLaunch tg) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nrec = fr.n_recs;

    uint32_t* scratch = smem;
    InterpTracer<kCount> tr;
    if constexpr (kProgInLds) {
        const uint4* src = reinterpret_cast<const uint4*>(gprog);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        for (uint32_t i = tid; i < nrec * 2u; i += kBlock) dst[i] = src[i];
        __syncthreads();
        tr.prog.p = reinterpret_cast<const WoRec*>(smem);
        scratch = smem + nrec * 8u;
    } else {
        tr.prog.p = gprog;
    }
    uint32_t* ws = scratch + wave * lay.wave_words;
    tr.nrec = nrec;
    tr.codes = ws;
    tr.ordpc = ws + lay.ordpc_off;
    tr.hib = ws + lay.hib_off;
    tr.lane = lane;
    pathtrace_block(tr, mats, fr, local_rows, out, seg_slots, tg);
}

// ---------------------------------------------------------------------------
// Ray queries (wo_renderer_trace_rays_device): the tracers above on the caller's
// rays instead of camera jobs.  A ray is two float4 (origin | t_max, dir |
// reserved: Wo_Ray), a hit two float4 (t, flags, leaf, node | normal, material:
// Wo_RayHit); one ray per lane, grid-stride over a grid of resident workgroups,
// so the workgroup's prologue (program / top BVH nodes into LDS) is paid once
// for many rays.
// ---------------------------------------------------------------------------
constexpr uint32_t kRayHit = 1u, kRayExit = 2u, kRayEnters = 4u, kRayInvalid = 8u;  // WO_RAY_* (renderer_ext.h)

struct RayBatch {
    const float4* __restrict__ rays;
    float4* __restrict__ hits;
    const uint32_t* __restrict__ nodes;  // per program record: its source node handle
    uint64_t n;
    uint32_t n_mats;
};

// Finite origin and direction, a direction that is not zero, t_max not NaN
// (t_max = -inf is a valid ray that no hit satisfies).
__device__ __forceinline__ bool ray_valid(const float4& r0, const float4& r1) {
    const bool fin = (fabsf(r0.x) < kInf) & (fabsf(r0.y) < kInf) & (fabsf(r0.z) < kInf) & (fabsf(r1.x) < kInf) &
                     (fabsf(r1.y) < kInf) & (fabsf(r1.z) < kInf);
    const bool nonzero = (r1.x != 0.0f) | (r1.y != 0.0f) | (r1.z != 0.0f);
    return fin & nonzero & !(r0.w != r0.w);
}

// Ray i's result: a hit (`found`: the root flips at h.t <= t_max; `leaf` = the hit
// member's record) with the solid's outward normal as the path tracer's NORMALS
// shading forms it (oracle.c shade_pixel), or the miss encoding.
__device__ __forceinline__ void ray_store(const RayBatch& rb, const WoRec* __restrict__ prog, uint64_t i, bool valid,
                                          bool found, const Hit& h, uint32_t leaf, F3 o, F3 d) {
    float4 h0 = make_float4(kInf, __uint_as_float(valid ? 0u : kRayInvalid), __uint_as_float(0xffffffffu),
                            __uint_as_float(0xffffffffu));
    float4 h1 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
    if (found) {
        const WoRec L = prog[leaf];
        const F3 P = f3(o.x + h.t * d.x, o.y + h.t * d.y, o.z + h.t * d.z);
        F3 n;
        if (L.op == WO_LEAF_SPHERE)
            n = f3((P.x - L.f[0]) * L.f[4], (P.y - L.f[1]) * L.f[4], (P.z - L.f[2]) * L.f[4]);
        else
            n = f3(L.f[0], L.f[1], L.f[2]);
        const F3 N = h.type() == 0u ? n : f3(-n.x, -n.y, -n.z);
        const F3 ns = h.root_after != 0u ? N : f3(-N.x, -N.y, -N.z);
        const uint32_t flags = kRayHit | (h.type() ? kRayExit : 0u) | (h.root_after ? kRayEnters : 0u);
        h0 = make_float4(h.t, __uint_as_float(flags), __uint_as_float(leaf), __uint_as_float(rb.nodes[leaf]));
        h1 = make_float4(ns.x, ns.y, ns.z, __uint_as_float(L.u0 < rb.n_mats ? L.u0 : 0u));
    }
    rb.hits[2u * i] = h0;
    rb.hits[2u * i + 1u] = h1;
}

// The interpreter over rays (any scene).  Its walk is wave-uniform, so every lane
// of a tracing wave needs a ray: lanes past n and lanes with an invalid ray trace
// a copy of the wave's first valid ray and drop the result (a copy adds no BOUND
// the wave would not enter anyway, and a lane's events are its own: a ray's result
// does not depend on its wave-mates); a wave without a valid ray skips the trace.
// The hit's ordinal counts the primitives the wave kept; its record index comes
// from the wave's own ordinal -> pc map.
template <bool kProgInLds>
__global__ __launch_bounds__(kBlock) void trace_rays_kernel(const WoRec* __restrict__ gprog, uint32_t nrec,
                                                            KLayout lay, RayBatch rb) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uni(tid >> 6);

    uint32_t* scratch = smem;
    InterpTracer<false> tr;
    if constexpr (kProgInLds) {
        const uint4* src = reinterpret_cast<const uint4*>(gprog);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        for (uint32_t i = tid; i < nrec * 2u; i += kBlock) dst[i] = src[i];
        __syncthreads();
        tr.prog.p = reinterpret_cast<const WoRec*>(smem);
        scratch = smem + nrec * 8u;
    } else {
        tr.prog.p = gprog;
    }
    uint32_t* ws = scratch + wave * lay.wave_words;
    tr.nrec = nrec;
    tr.codes = ws;
    tr.ordpc = ws + lay.ordpc_off;
    tr.hib = ws + lay.hib_off;
    tr.lane = lane;

    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock + wave * 64u; base < rb.n; base += stride) {
        const uint64_t i = base + lane;
        const bool in = i < rb.n;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;
        if (in) {
            r0 = rb.rays[2u * i];
            r1 = rb.rays[2u * i + 1u];
        }
        const bool valid = in && ray_valid(r0, r1);
        const uint64_t vm = __ballot(valid);
        const F3 o = f3(r0.x, r0.y, r0.z), d = f3(r1.x, r1.y, r1.z);
        bool found = false;
        uint32_t leaf = 0;
        Hit h;
        h.t = kInf;
        h.lo = 0;
        h.root_after = 0;
        if (vm != 0ull) {
            const int src = __builtin_ctzll(vm);
            auto from = [&](float v) { return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), src)); };
            const F3 so = f3(from(o.x), from(o.y), from(o.z)), sd = f3(from(d.x), from(d.y), from(d.z));
            const F3 to = valid ? o : so, td = valid ? d : sd;
            found = tr.trace(to, td, h);
            found = found & valid & (h.t <= r0.w);
            if (found) leaf = tr.ordpc[h.ord()] + 1u + h.member();
        }
        if (in) ray_store(rb, gprog, i, valid, found, h, leaf, o, d);
    }
}

// The lane tracer's ordered BVH walk over rays (union-only scenes; forms 2 and 3 of
// pathtrace_lanes_kernel, the plain trace).  Every lane walks on its own, so a lane
// without a valid ray simply does not trace.
template <int kMode>
__global__ __launch_bounds__(kBlock, kMode == 2 ? WO_LANES_BVH_MIN_WAVES : WO_LANES_MIN_WAVES) void trace_rays_lanes_kernel(
    const WoRec* __restrict__ prog, const uint32_t* __restrict__ ordpc, LaneBvh bvh, RayBatch rb) {
    static_assert(kMode == 2 || kMode == 3, "ray queries walk the union-only forms");
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    LaneTracer<kMode, false> tr;
    tr.prog = prog;
    tr.ordpc = ordpc;
    tr.lnodes = bvh.nodes;
    tr.lgeo = bvh.geo;
    tr.lkind = bvh.kind;
    tr.ltrec = bvh.trec;
    tr.lleaf = bvh.leaves;
    tr.nalways = bvh.nalways;
    tr.lroot = bvh.root;
    tr.nprims = bvh.nprims;
    tr.stk = smem + threadIdx.x;
    tr.stk16 = reinterpret_cast<uint16_t*>(smem) + threadIdx.x;
    {
        // the top levels of the BVH next to the stacks, as pathtrace_lanes_kernel lays them out
        float4* top = reinterpret_cast<float4*>(smem + ((bvh.depth * kBlock + 3u) & ~3u));
        for (uint32_t i = threadIdx.x; i < 4u * bvh.ntop; i += kBlock) top[i] = bvh.nodes[i];
        tr.ltop = (typename LaneTracer<kMode, false>::LdsNodes)top;
        tr.ntop = bvh.ntop;
    }
    __syncthreads();

    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < rb.n; i += stride) {
        const float4 r0 = rb.rays[2u * i], r1 = rb.rays[2u * i + 1u];
        const bool valid = ray_valid(r0, r1);
        const F3 o = f3(r0.x, r0.y, r0.z), d = f3(r1.x, r1.y, r1.z);
        bool found = false;
        uint32_t leaf = 0;
        Hit h;
        h.t = kInf;
        h.lo = 0;
        h.root_after = 0;
        if (valid) {
            found = tr.trace(o, d, h);
            found = found & (h.t <= r0.w);
            if (found) leaf = ordpc[h.ord()] + 1u + h.member();
        }
        ray_store(rb, prog, i, valid, found, h, leaf, o, d);
    }
}

// ---------------------------------------------------------------------------
// First-hit feature buffers (wo_renderer_render_features_device): per pixel the mean
// albedo, facing normal and depth of the first hits of the frame's own camera rays,
// the coverage, and the ids under the pixel centre (renderer_ext.h states the
// semantics).  No ray is read: a lane makes sample s of its pixel in registers, as
// pathtrace_block's job_ray does, traces it and adds to seven exact 32.32 sums and a
// hit count that stay in registers; it then stores one 16-byte row per plane.  The
// only other global traffic is the program, the materials and the node table.
// ---------------------------------------------------------------------------
struct FeatureLaunch {
    WoFrame fr;
    const WoMaterial* __restrict__ mats;
    const uint32_t* __restrict__ nodes;  // per program record: its source node handle
    uint4* __restrict__ out;
    uint64_t plane_stride;               // 16-byte rows between two planes
    uint32_t local_rows, n_mats;
};

// The camera ray of sample s of frame pixel (x, y): job_ray (wo_device_common.h) and the
// unit3 that follows its take, restated for one pixel per lane.  `centre`: the pixel
// centre without jitter or lens, the NORMALS sample (wo_renderer_pixel_ray).
__device__ __forceinline__ void feature_ray(const WoFrame& fr, uint32_t seed_hash, uint32_t x, uint32_t y, uint32_t s,
                                            bool centre, F3& o, F3& d) {
    const WoCamera& cam = fr.cam;
    Rng nr;
    nr.s = pcg_hash((y * fr.width + x) ^ pcg_hash((fr.sample_offset + s) ^ seed_hash));
    float sx, ty;
    if (centre) {
        sx = ((float)x + 0.5f) * fr.inv_width;
        ty = ((float)(fr.height - 1u - y) + 0.5f) * fr.inv_height;
    } else {
        float r1 = nr.uniform();
        float r2 = nr.uniform();
        sx = ((float)x + r1) * fr.inv_width;
        ty = ((float)(fr.height - 1u - y) + r2) * fr.inv_height;
    }
    float offx = 0.0f, offy = 0.0f, offz = 0.0f;
    if (cam.lens_radius > 0.0f && !centre) {
        // uniform point on the unit disk: radius sqrt(u), angle 2*pi*v
        float rr = sqrt_pt(nr.uniform());
        float sn, cs;
        sincos_turns(nr.uniform(), sn, cs);
        float px = rr * cs, py = rr * sn;
        float rx = cam.lens_radius * px, ry = cam.lens_radius * py;
        offx = cam.u[0] * rx + cam.v[0] * ry;
        offy = cam.u[1] * rx + cam.v[1] * ry;
        offz = cam.u[2] * rx + cam.v[2] * ry;
    }
    o = f3(cam.origin[0] + offx, cam.origin[1] + offy, cam.origin[2] + offz);
    d = unit3(f3(((cam.lower_left[0] + sx * cam.horizontal[0]) + ty * cam.vertical[0]) - cam.origin[0] - offx,
                 ((cam.lower_left[1] + sx * cam.horizontal[1]) + ty * cam.vertical[1]) - cam.origin[1] - offy,
                 ((cam.lower_left[2] + sx * cam.horizontal[2]) + ty * cam.vertical[2]) - cam.origin[2] - offz));
}

// A pixel's sums: albedo, facing normal (0 on a miss) and the hits' t, each sample
// quantised as the frame's radiance is, so the means do not depend on sample order.
struct FeatureSums {
    long long a[3], n[3], t;
    uint32_t hits;
};

// One sample's first hit (`L`: the hit member's leaf record) or miss added to the sums.
__device__ __forceinline__ void feature_add(FeatureSums& fs, const FeatureLaunch& fl, bool found, const Hit& h,
                                            const WoRec& L, F3 o, F3 d) {
    F3 a;
    if (found) {
        const F3 P = f3(o.x + h.t * d.x, o.y + h.t * d.y, o.z + h.t * d.z);
        F3 n;
        if (L.op == WO_LEAF_SPHERE)
            n = f3((P.x - L.f[0]) * L.f[4], (P.y - L.f[1]) * L.f[4], (P.z - L.f[2]) * L.f[4]);
        else
            n = f3(L.f[0], L.f[1], L.f[2]);
        const F3 N = h.type() == 0u ? n : f3(-n.x, -n.y, -n.z);
        const F3 ns = h.root_after != 0u ? N : f3(-N.x, -N.y, -N.z);
        const WoMaterial m = fl.mats[L.u0 < fl.n_mats ? L.u0 : 0u];
        const bool diel = (m.kind != WO_MAT_LAMBERTIAN) & (m.kind != WO_MAT_METAL);
        a = diel ? f3(1.0f, 1.0f, 1.0f) : f3(m.albedo[0], m.albedo[1], m.albedo[2]);
        fs.n[0] += quantize_radiance(ns.x);
        fs.n[1] += quantize_radiance(ns.y);
        fs.n[2] += quantize_radiance(ns.z);
        fs.t += quantize_radiance(h.t);
        ++fs.hits;
    } else {
        a = sky(d);
    }
    fs.a[0] += quantize_radiance(a.x);
    fs.a[1] += quantize_radiance(a.y);
    fs.a[2] += quantize_radiance(a.z);
}

// The pixel's three rows: plane p of local pixel i is row p * plane_stride + i.
__device__ __forceinline__ void feature_store(const FeatureLaunch& fl, size_t i, const FeatureSums& fs, uint4 ids) {
    const uint32_t spp = fl.fr.spp;
    const float cover = (float)((double)fs.hits / (double)spp);
    const float depth = fs.hits ? mean_radiance(fs.t, fs.hits) : kInf;
    float4* out = reinterpret_cast<float4*>(fl.out);
    out[i] = make_float4(mean_radiance(fs.a[0], spp), mean_radiance(fs.a[1], spp), mean_radiance(fs.a[2], spp), cover);
    out[fl.plane_stride + i] =
        make_float4(mean_radiance(fs.n[0], spp), mean_radiance(fs.n[1], spp), mean_radiance(fs.n[2], spp), depth);
    fl.out[2u * fl.plane_stride + i] = ids;
}

// Wo_FeatureIds of the centre ray's result (leaf = the hit member's record index).
__device__ __forceinline__ uint4 feature_ids(const FeatureLaunch& fl, bool found, const Hit& h, const WoRec& L,
                                             uint32_t leaf) {
    if (!found) return make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0u);
    const uint32_t flags = kRayHit | (h.type() ? kRayExit : 0u) | (h.root_after ? kRayEnters : 0u);
    return make_uint4(fl.nodes[leaf], leaf, L.u0 < fl.n_mats ? L.u0 : 0u, flags);
}

// A wave's item of 64 pixels of the rank's local rows: an 8 x 8 tile (lane = 8 row +
// column) or a 64 x 1 strip of one row, numbered row-major and dealt to the waves by
// the grid-stride loop.  Both were measured; the planes do not depend
// on the footprint.
template <bool kTile>
struct FeatureItems {
    uint32_t across;
    uint64_t count;
    __device__ __forceinline__ FeatureItems(uint32_t width, uint32_t rows) {
        across = kTile ? (width + 7u) >> 3 : (width + 63u) >> 6;
        count = (uint64_t)across * (kTile ? (rows + 7u) >> 3 : rows);
    }
    __device__ __forceinline__ void pixel(uint64_t item, uint32_t lane, uint32_t& lx, uint32_t& lrow) const {
        const uint32_t iy = (uint32_t)(item / across), ix = (uint32_t)(item - (uint64_t)iy * across);
        lx = ix * (kTile ? 8u : 64u) + (kTile ? (lane & 7u) : lane);
        lrow = iy * (kTile ? 8u : 1u) + (kTile ? (lane >> 3) : 0u);
    }
};

// The interpreter over the frame's camera rays (any scene): the wave traces sample s
// of its 64 pixels together, which suits the wave-uniform walk as camera waves suit
// the frame kernel.  A lane whose pixel is outside the frame (past the right edge, or
// a local row beyond the frame's last) traces the wave's first in-frame pixel and
// drops the result; a wave without an in-frame pixel skips the item.
template <bool kProgInLds, bool kTile>
__global__ __launch_bounds__(kBlock) void features_kernel(const WoRec* __restrict__ gprog, uint32_t nrec, KLayout lay,
                                                          FeatureLaunch fl) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uni(tid >> 6);

    uint32_t* scratch = smem;
    InterpTracer<false> tr;
    if constexpr (kProgInLds) {
        const uint4* src = reinterpret_cast<const uint4*>(gprog);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        for (uint32_t i = tid; i < nrec * 2u; i += kBlock) dst[i] = src[i];
        __syncthreads();
        tr.prog.p = reinterpret_cast<const WoRec*>(smem);
        scratch = smem + nrec * 8u;
    } else {
        tr.prog.p = gprog;
    }
    uint32_t* ws = scratch + wave * lay.wave_words;
    tr.nrec = nrec;
    tr.codes = ws;
    tr.ordpc = ws + lay.ordpc_off;
    tr.hib = ws + lay.hib_off;
    tr.lane = lane;

    const uint32_t W = fl.fr.width, H = fl.fr.height, spp = fl.fr.spp;
    const uint32_t seed_hash = pcg_hash(fl.fr.seed);
    const FeatureItems<kTile> items(W, fl.local_rows);
    const uint64_t stride = (uint64_t)gridDim.x * (kBlock / 64u);
    for (uint64_t item = (uint64_t)blockIdx.x * (kBlock / 64u) + wave; item < items.count; item += stride) {
        uint32_t lx, lrow;
        items.pixel(item, lane, lx, lrow);
        const uint32_t gy = lrow < fl.local_rows ? local_to_global_row(fl.fr, lrow) : H;
        const bool in = lx < W && gy < H;
        const uint64_t vm = __ballot(in);
        if (vm == 0ull) continue;
        const int src = __builtin_ctzll(vm);
        const uint32_t x = in ? lx : (uint32_t)__builtin_amdgcn_readlane((int)lx, src);
        const uint32_t y = in ? gy : (uint32_t)__builtin_amdgcn_readlane((int)gy, src);
        FeatureSums fs = {};
        uint4 ids = make_uint4(0u, 0u, 0u, 0u);
        // samples 0 .. spp - 1, then the centre ray (one call site of the tracer; ends for every spp)
        for (uint32_t s = 0;; ++s) {
            const bool centre = s == spp;
            F3 o, d;
            feature_ray(fl.fr, seed_hash, x, y, s, centre, o, d);
            Hit h;
            h.t = kInf;
            h.lo = 0;
            h.root_after = 0;
            const bool found = tr.trace(o, d, h);
            WoRec L = {};
            uint32_t leaf = 0;
            if (found) {
                leaf = tr.ordpc[h.ord()] + 1u + h.member();
                L = tr.prog[leaf];
            }
            if (centre) {
                ids = feature_ids(fl, found, h, L, leaf);
                break;
            }
            feature_add(fs, fl, found, h, L, o, d);
        }
        if (in) feature_store(fl, (size_t)lrow * W + lx, fs, ids);
    }
}

// The lane tracer's ordered BVH walk over the same rays (union-only scenes; forms 2
// and 3, trace_rays_lanes_kernel's prologue).  Every lane walks on its own, so a lane
// whose pixel is outside the frame does nothing.  Five and six waves per SIMD, not the
// ray kernels' seven and eight: the sums are 15 registers the walk does not have, and
// under the ray kernels' bounds (72 / 64 VGPRs) they spill 72 bytes of scratch per lane.
template <int kMode, bool kTile>
__global__ __launch_bounds__(kBlock, kMode == 2 ? 5 : 6) void features_lanes_kernel(
    const WoRec* __restrict__ prog, const uint32_t* __restrict__ ordpc, LaneBvh bvh, FeatureLaunch fl) {
    static_assert(kMode == 2 || kMode == 3, "feature buffers walk the union-only forms");
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    LaneTracer<kMode, false> tr;
    tr.prog = prog;
    tr.ordpc = ordpc;
    tr.lnodes = bvh.nodes;
    tr.lgeo = bvh.geo;
    tr.lkind = bvh.kind;
    tr.ltrec = bvh.trec;
    tr.lleaf = bvh.leaves;
    tr.nalways = bvh.nalways;
    tr.lroot = bvh.root;
    tr.nprims = bvh.nprims;
    tr.stk = smem + threadIdx.x;
    tr.stk16 = reinterpret_cast<uint16_t*>(smem) + threadIdx.x;
    {
        // the top levels of the BVH next to the stacks, as pathtrace_lanes_kernel lays them out
        float4* top = reinterpret_cast<float4*>(smem + ((bvh.depth * kBlock + 3u) & ~3u));
        for (uint32_t i = threadIdx.x; i < 4u * bvh.ntop; i += kBlock) top[i] = bvh.nodes[i];
        tr.ltop = (typename LaneTracer<kMode, false>::LdsNodes)top;
        tr.ntop = bvh.ntop;
    }
    __syncthreads();

    const uint32_t W = fl.fr.width, H = fl.fr.height, spp = fl.fr.spp;
    const uint32_t seed_hash = pcg_hash(fl.fr.seed);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const FeatureItems<kTile> items(W, fl.local_rows);
    const uint64_t stride = (uint64_t)gridDim.x * (kBlock / 64u);
    for (uint64_t item = (uint64_t)blockIdx.x * (kBlock / 64u) + wave; item < items.count; item += stride) {
        uint32_t x, lrow;
        items.pixel(item, lane, x, lrow);
        const uint32_t y = lrow < fl.local_rows ? local_to_global_row(fl.fr, lrow) : H;
        if (!(x < W && y < H)) continue;
        FeatureSums fs = {};
        uint4 ids = make_uint4(0u, 0u, 0u, 0u);
        for (uint32_t s = 0;; ++s) {
            const bool centre = s == spp;
            F3 o, d;
            feature_ray(fl.fr, seed_hash, x, y, s, centre, o, d);
            Hit h;
            h.t = kInf;
            h.lo = 0;
            h.root_after = 0;
            const bool found = tr.trace(o, d, h);
            WoRec L = {};
            uint32_t leaf = 0;
            if (found) {
                leaf = ordpc[h.ord()] + 1u + h.member();
                L = prog[leaf];
            }
            if (centre) {
                ids = feature_ids(fl, found, h, L, leaf);
                break;
            }
            feature_add(fs, fl, found, h, L, o, d);
        }
        feature_store(fl, (size_t)lrow * W + x, fs, ids);
    }
}

// ---------------------------------------------------------------------------
// Ray span queries (wo_renderer_trace_spans_device): the interpreter's sweep carried
// on past the first flip of the root.  Every flip in (WO_T_MIN, t_max] is a crossing;
// a ray's summary is Wo_RaySpans (count, flags, length, stored: one uint4), a crossing
// Wo_RayCrossing (t, flags, leaf, node: one float4), stored crossing-major
// (crossing k of ray i at [k * n + i]: a wave's k-th store is 64 consecutive rows).
// ---------------------------------------------------------------------------
constexpr uint32_t kRayInside = 16u, kRayTruncated = 32u;  // WO_RAY_INSIDE, WO_RAY_TRUNCATED

// Window's sorted network at another size (Window itself is the specialised kernels'
// too and stays as it is): the kN nearest events, the largest dropped on overflow.
template <int kN>
struct SpanWindow {
    static_assert(WO_WIN_F64, "the network is Window's v_min_f64 / v_max_f64 one");
    static constexpr uint64_t kEmpty = Window::kEmpty;
    uint64_t k[kN];
    uint32_t n;  // inserts since clear()
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < kN; ++i) k[i] = kEmpty;
        n = 0;
    }
    __device__ __forceinline__ bool dropped() const { return n > (uint32_t)kN; }
    __device__ __forceinline__ bool empty() const { return k[0] == kEmpty; }
    __device__ __forceinline__ void insert(uint64_t key) {
        ++n;
#pragma unroll
        for (int i = kN - 1; i > 0; --i) k[i] = key_max(k[i - 1], key_min(key, k[i]));
        k[0] = key_min(key, k[0]);
    }
    __device__ __forceinline__ uint64_t pop() {
        uint64_t r = k[0];
#pragma unroll
        for (int i = 0; i < kN - 1; ++i) k[i] = k[i + 1];
        k[kN - 1] = kEmpty;
        return r;
    }
};

struct SpanBatch {
    const float4* __restrict__ rays;
    uint4* __restrict__ spans;
    float4* __restrict__ crossings;      // [max_crossings][n], or null when max_crossings = 0
    const uint32_t* __restrict__ nodes;  // per program record: its source node handle
    uint64_t n;
    uint32_t max_crossings;
};

// A ray's sweep state: what Wo_RaySpans reports, in the making.
struct SpanSum {
    uint32_t count;
    uint32_t inside0;  // the root's value at WO_T_MIN
    uint32_t root;     // the root's value after the last swept event
    float len, t_in;
};

// The interpreter's trace as a span query.  Pass 1 is trace()'s.  Pass 2 sweeps the
// events in key order and calls crossing(key, root_after, k) at the k-th flip of the
// root instead of returning at the first one; it re-collects strictly after the last
// swept key whenever the window ran empty after dropping events.  An event later than
// t_max ends the sweep (no later event can be a crossing).
// Termination: a re-collect admits only keys greater than the last swept one, each
// window holds at least one of them, and a ray has at most two events per primitive;
// so every key is swept at most once and the loop needs no iteration cap.
// The result does not depend on kN: the windows only batch one sorted sequence.
template <int kN, class Crossing>
__device__ __forceinline__ SpanSum trace_spans(InterpTracer<false>& tr, F3 o, F3 d, float t_max, Crossing&& crossing) {
    SpanWindow<kN> win;
    win.clear();
    F3 inv = f3(0.0f, 0.0f, 0.0f);
    bool have_inv = false;
    SpanSum s;
    s.root = s.inside0 = tr.collect(o, d, win, inv, have_inv) & 1u;
    s.count = 0;
    s.len = 0.0f;
    s.t_in = WO_T_MIN;
    while (!win.empty()) {
        const uint64_t key = win.pop();
        const float t = __uint_as_float((uint32_t)(key >> 32));
        if (t > t_max) break;
        tr.toggle(key_ord(key));
        const uint32_t r = tr.eval_root();
        if (r != s.root) {
            crossing(key, r, s.count);
            ++s.count;
            // fp32, one rounding per operation, in sweep order (Wo_RaySpans.length)
            if (r)
                s.t_in = t;
            else
                s.len = s.len + (t - s.t_in);
            s.root = r;
        }
        if (win.empty() && win.dropped()) tr.recollect(o, d, key, win, inv, have_inv);
    }
    if (s.root && t_max > s.t_in) s.len = s.len + (t_max - s.t_in);
    return s;
}

// One ray per lane, the grid and LDS layout of trace_rays_kernel; lanes past n and
// lanes with an invalid ray sweep a copy of the wave's first valid ray (t_max too)
// and drop the result.
template <bool kProgInLds, int kN>
__global__ __launch_bounds__(kBlock) void trace_spans_kernel(const WoRec* __restrict__ gprog, uint32_t nrec,
                                                             KLayout lay, SpanBatch sb) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uni(tid >> 6);

    uint32_t* scratch = smem;
    InterpTracer<false> tr;
    if constexpr (kProgInLds) {
        const uint4* src = reinterpret_cast<const uint4*>(gprog);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        for (uint32_t i = tid; i < nrec * 2u; i += kBlock) dst[i] = src[i];
        __syncthreads();
        tr.prog.p = reinterpret_cast<const WoRec*>(smem);
        scratch = smem + nrec * 8u;
    } else {
        tr.prog.p = gprog;
    }
    uint32_t* ws = scratch + wave * lay.wave_words;
    tr.nrec = nrec;
    tr.codes = ws;
    tr.ordpc = ws + lay.ordpc_off;
    tr.hib = ws + lay.hib_off;
    tr.lane = lane;

    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock + wave * 64u; base < sb.n; base += stride) {
        const uint64_t i = base + lane;
        const bool in = i < sb.n;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;
        if (in) {
            r0 = sb.rays[2u * i];
            r1 = sb.rays[2u * i + 1u];
        }
        const bool valid = in && ray_valid(r0, r1);
        const uint64_t vm = __ballot(valid);
        SpanSum s;
        s.count = 0;
        s.inside0 = s.root = 0;
        s.len = 0.0f;
        s.t_in = WO_T_MIN;
        if (vm != 0ull) {
            const int src = __builtin_ctzll(vm);
            auto from = [&](float v) { return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), src)); };
            const F3 so = f3(from(r0.x), from(r0.y), from(r0.z)), sd = f3(from(r1.x), from(r1.y), from(r1.z));
            const float st_max = from(r0.w);
            const F3 to = valid ? f3(r0.x, r0.y, r0.z) : so, td = valid ? f3(r1.x, r1.y, r1.z) : sd;
            s = trace_spans<kN>(tr, to, td, valid ? r0.w : st_max, [&](uint64_t key, uint32_t root_after, uint32_t k) {
                if (!valid || k >= sb.max_crossings) return;
                const uint32_t lo = (uint32_t)key;
                const uint32_t leaf = tr.ordpc[lo >> 12] + 1u + (lo & 2047u);
                const uint32_t flags = kRayHit | ((lo & kKeyTypeBit) ? kRayExit : 0u) | (root_after ? kRayEnters : 0u);
                sb.crossings[(uint64_t)k * sb.n + i] =
                    make_float4(__uint_as_float((uint32_t)(key >> 32)), __uint_as_float(flags), __uint_as_float(leaf),
                                __uint_as_float(sb.nodes[leaf]));
            });
        }
        if (in) {
            uint4 out = make_uint4(0u, kRayInvalid, 0u, 0u);
            if (valid) {
                const uint32_t stored = s.count < sb.max_crossings ? s.count : sb.max_crossings;
                const uint32_t flags = (s.inside0 ? kRayInside : 0u) | (s.count > stored ? kRayTruncated : 0u);
                out = make_uint4(s.count, flags, __float_as_uint(s.len), stored);
            }
            sb.spans[i] = out;
        }
    }
}

// ---------------------------------------------------------------------------
// Mass properties (wo_renderer_mass_sums_device): a grid of parallel rays made in
// registers from the plan (renderer_ext.h Wo_MassPlan), each span quantised and
// integrated as trace_spans sweeps it, the ten sums and three counters of
// Wo_MassSums accumulated as exact integers.  No ray is read and no row written:
// a workgroup's only traffic to global memory, the program apart, is up to 23 64-bit
// atomic adds at its end.
// ---------------------------------------------------------------------------
constexpr int kMassSlots = 23;  // Wo_MassSums: lo[10], hi[10], rays, rays_hit, crossings (reserved is not touched)
static_assert(0x1p-9f > WO_T_MIN, "Wo_MassPlan.pad: a surface on the near face must be a crossing");

// Where the accumulators live between a lane's rays (measured; the sums
// are the same integers whichever is used):
//   kMassRegs   per lane in registers over the whole loop, reduced once at the end;
//   kMassShfl   reduced across the wave after every ray, kept wave-uniform;
//   kMassLds    every lane adds into its wave's slots in LDS (64-bit ds_add).
enum { kMassRegs = 0, kMassShfl = 1, kMassLds = 2 };

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    return v;
}
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
    return ((uint64_t)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v);
}

// kTile: a wave takes an 8 x 8 tile of cells (lane = 8 row + column), else a 64 x 1
// strip of one row.  Items (tiles or strips) are numbered row-major over the row
// range and dealt to the waves by the grid-stride loop; lane 0 of an item is always
// a cell of the grid.
template <bool kProgInLds, int kN, bool kTile, int kRed>
__global__ __launch_bounds__(kBlock) void mass_grid_kernel(const WoRec* __restrict__ gprog, uint32_t nrec, KLayout lay,
                                                           WoMassLaunch ml, unsigned long long* __restrict__ sums,
                                                           uint32_t block_flush) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uni(tid >> 6);

    uint32_t* scratch = smem;
    InterpTracer<false> tr;
    if constexpr (kProgInLds) {
        const uint4* src = reinterpret_cast<const uint4*>(gprog);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        for (uint32_t i = tid; i < nrec * 2u; i += kBlock) dst[i] = src[i];
        __syncthreads();
        tr.prog.p = reinterpret_cast<const WoRec*>(smem);
        scratch = smem + nrec * 8u;
    } else {
        tr.prog.p = gprog;
    }
    uint32_t* ws = scratch + wave * lay.wave_words;
    tr.nrec = nrec;
    tr.codes = ws;
    tr.ordpc = ws + lay.ordpc_off;
    tr.hib = ws + lay.hib_off;
    tr.lane = lane;

    uint64_t acc[kMassSlots];
#pragma unroll
    for (int s = 0; s < kMassSlots; ++s) acc[s] = 0ull;
    // (a static array beside the dynamic one; only the kMassLds instantiations have it)
    unsigned long long* slots = nullptr;
    if constexpr (kRed == kMassLds) {
        __shared__ unsigned long long mass_slots[kBlock / 64u][kMassSlots + 1];
        slots = mass_slots[wave];
        if (lane < (uint32_t)kMassSlots) slots[lane] = 0ull;  // the wave's own slots: no barrier needed
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }

    const uint32_t across = kTile ? (ml.nu + 7u) >> 3 : (ml.nu + 63u) >> 6;
    const uint32_t down = kTile ? (ml.v_count + 7u) >> 3 : ml.v_count;
    const uint64_t items = (uint64_t)across * down;
    const uint32_t li = kTile ? (lane & 7u) : lane, lj = kTile ? (lane >> 3) : 0u;
    const uint64_t stride = (uint64_t)gridDim.x * (kBlock / 64u);
    for (uint64_t item = (uint64_t)blockIdx.x * (kBlock / 64u) + wave; item < items; item += stride) {
        const uint32_t iy = (uint32_t)(item / across), ix = (uint32_t)(item - (uint64_t)iy * across);
        const uint32_t ci = ix * (kTile ? 8u : 64u) + li, cj = iy * (kTile ? 8u : 1u) + lj;
        const bool in = ci < ml.nu && cj < ml.v_count;
        // lanes past the grid's edge sweep lane 0's ray (always a cell) and drop the result
        const uint32_t i = in ? ci : uni(ci), j = ml.v_begin + (in ? cj : uni(cj));
        const uint32_t i2 = 2u * i + 1u, j2 = 2u * j + 1u;
        // two roundings each: the product, then the sum (no contraction in this file)
        const float pu = (float)i2 * ml.hu, pv = (float)j2 * ml.hv;
        const float cu = ml.u0 + pu, cv = ml.v0 + pv;
        F3 o, d;
        if (ml.axis == 0u) {
            o = f3(ml.o_axis, cu, cv);
            d = f3(1.0f, 0.0f, 0.0f);
        } else if (ml.axis == 1u) {
            o = f3(cv, ml.o_axis, cu);
            d = f3(0.0f, 1.0f, 0.0f);
        } else {
            o = f3(cu, cv, ml.o_axis);
            d = f3(0.0f, 0.0f, 1.0f);
        }
        uint32_t qa = ml.q0, m0 = 0u;
        uint64_t m1 = 0ull, m2 = 0ull;
        auto close = [&](uint32_t qb) {  // the span [qa, qb]: qa <= qb <= 2^20, so a^3 <= 2^60
            const uint64_t a = qa, b = qb;
            m0 += qb - qa;
            m1 += b * b - a * a;
            m2 += b * b * b - a * a * a;
        };
        const SpanSum s = trace_spans<kN>(tr, o, d, ml.t_max, [&](uint64_t key, uint32_t root_after, uint32_t) {
            const float t = __uint_as_float((uint32_t)(key >> 32));
            const uint32_t q = (uint32_t)rintf(t * ml.scale);  // exact product, half to even
            const uint32_t c = min(max(q, ml.q0), ml.q1);
            if (root_after)
                qa = c;
            else
                close(c);
        });
        if (s.root) close(ml.q1);
        // a ray's ten terms, each below 2^63, split into 32-bit limbs (Wo_MassSums): with at
        // most 2^31 rays added into one buffer a limb sum stays below 2^31 * 2^32 = 2^63
        auto accumulate = [&](int k, uint64_t v) {
            if constexpr (kRed == kMassRegs)
                acc[k] += v;
            else if constexpr (kRed == kMassShfl)
                acc[k] += uni64(wave_sum(v));
            else if (v != 0ull)
                (void)atomicAdd(&slots[k], (unsigned long long)v);
        };
        // (m0 = 0 leaves m1 = m2 = 0: a wave none of whose rays met the solid adds counters only)
        if (__ballot(in && m0 != 0u) != 0ull) {
            const uint64_t w0 = in ? m0 : 0u, w1 = in ? m1 : 0ull, w2 = in ? m2 : 0ull;
            const uint64_t term[10] = {w0,           w0 * i2, w0 * j2,      w1,      w0 * i2 * i2,
                                       w0 * j2 * j2, w2,      w0 * i2 * j2, w1 * i2, w1 * j2};
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                accumulate(k, term[k] & 0xFFFFFFFFull);
                accumulate(10 + k, term[k] >> 32);
            }
        }
        accumulate(20, in ? 1ull : 0ull);
        accumulate(21, in && m0 > 0u ? 1ull : 0ull);
        accumulate(22, in ? (uint64_t)s.count : 0ull);
    }
    if constexpr (kRed == kMassLds) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    uint64_t total[kMassSlots];  // the wave's, wave-uniform
#pragma unroll
    for (int k = 0; k < kMassSlots; ++k) {
        if constexpr (kRed == kMassRegs)
            total[k] = wave_sum(acc[k]);
        else if constexpr (kRed == kMassShfl)
            total[k] = acc[k];
        else
            total[k] = __hip_atomic_load(&slots[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);  // the wave's own adds
    }
    if (!block_flush) {  // one atomic add per slot and wave
#pragma unroll
        for (int k = 0; k < kMassSlots; ++k)
            if (lane == 0u && total[k] != 0ull) (void)atomicAdd(&sums[k], (unsigned long long)total[k]);
        return;
    }
    // One atomic add per slot and WORKGROUP: all of a launch's adds go to the same two
    // cache lines, where they are served one after another, so their number is what the
    // tail of the kernel costs.  The waves' totals meet in the dynamic LDS,
    // which the program and the scratch no longer need (the host sizes it for this too).
    __syncthreads();
    unsigned long long* red = reinterpret_cast<unsigned long long*>(smem);  // [waves][kMassSlots]
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < kMassSlots; ++k) red[wave * kMassSlots + k] = total[k];
    }
    __syncthreads();
    if (tid < (uint32_t)kMassSlots) {
        unsigned long long v = 0ull;
        for (uint32_t w = 0; w < kBlock / 64u; ++w) v += red[w * kMassSlots + tid];
        if (v != 0ull) (void)atomicAdd(&sums[tid], v);
    }
}
constexpr size_t kMassReduceLds = (kBlock / 64u) * kMassSlots * sizeof(unsigned long long);

// Point membership classification (wo_renderer_classify_points_device): one point
// (a float4, w ignored) per lane, the program walked once by the wave, the root
// evaluated on pass 1's bit stack.  Each leaf in fp32, one rounding per operation:
// sphere ((gx gx + gy gy) + gz gz) <= r^2 with g = p - c, half-space
// ((nx px + ny py) + nz pz) <= h; a primitive is the AND of its members.
// BOUND records are stepped over, never used to skip a subtree: skipping needs a
// margin by which every leaf test under the BOUND provably fails, and a BOUND taken
// from a polytope of half-spaces (scene_compile.c polytope_bound) gives none -- a point
// outside the bounding sphere by g may violate each plane near a sharp vertex by
// far less than g, down to the rounding of the plane test.  So the result is the
// evaluation that ignores BOUNDs by construction.
constexpr uint32_t kPointInside = 1u, kPointInvalid = 8u;  // WO_POINT_* (renderer_ext.h)

template <bool kProgInLds>
__global__ __launch_bounds__(kBlock) void classify_points_kernel(const WoRec* __restrict__ gprog, uint32_t nrec,
                                                                 const float4* __restrict__ points,
                                                                 uint32_t* __restrict__ out, uint64_t n) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    ProgPtr prog;
    if constexpr (kProgInLds) {
        const uint4* src = reinterpret_cast<const uint4*>(gprog);
        uint4* dst = reinterpret_cast<uint4*>(smem);
        for (uint32_t i = threadIdx.x; i < nrec * 2u; i += kBlock) dst[i] = src[i];
        __syncthreads();
        prog.p = reinterpret_cast<const WoRec*>(smem);
    } else {
        prog.p = gprog;
    }
    constexpr uint32_t kTruth = InterpTracer<false>::kTruth;
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    // (every lane of a wave runs the same trips: the bound is the wave's, the walk wave-uniform)
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u); base < n; base += stride) {
        const uint64_t i = base + (threadIdx.x & 63u);
        const bool in = i < n;
        const float4 p = in ? points[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        uint32_t st = 0;
        uint32_t pc = 0;
        while (pc < nrec) {
            const WoRec rec = prog[pc];
            const uint32_t op = uni(rec.op);
            if (op == WO_OP_BOUND) {
                ++pc;
            } else if (op == WO_OP_PRIM) {
                const uint32_t count = uni(rec.u0);
                bool inside = true;
                for (uint32_t m = 0; m < count; ++m) {
                    const WoRec L = prog[pc + 1u + m];
                    float v;
                    if (uni(L.op) == WO_LEAF_SPHERE) {
                        const float gx = p.x - L.f[0], gy = p.y - L.f[1], gz = p.z - L.f[2];
                        v = (gx * gx + gy * gy) + gz * gz;
                    } else {
                        v = (L.f[0] * p.x + L.f[1] * p.y) + L.f[2] * p.z;
                    }
                    inside = inside & (v <= L.f[3]);
                }
                st = (st << 1) | (inside ? 1u : 0u);
                pc += 1u + count;
            } else {
                const uint32_t tt = (kTruth >> (4u * op)) & 15u;
                st = ((st >> 2) << 1) | ((tt >> (st & 3u)) & 1u);
                ++pc;
            }
        }
        if (in) {
            const bool fin = (fabsf(p.x) < kInf) & (fabsf(p.y) < kInf) & (fabsf(p.z) < kInf);
            out[i] = fin ? ((st & 1u) ? kPointInside : 0u) : kPointInvalid;
        }
    }
}

// Sums (and clears) the segment slots into the caller's counter.
__global__ __launch_bounds__(kBlock) void seg_collect_kernel(unsigned long long* __restrict__ slots,
                                                             unsigned long long* __restrict__ counter) {
    __shared__ unsigned long long part[kBlock / 64];
    unsigned long long v = 0;
    for (uint32_t i = threadIdx.x; i < kSegSlots; i += kBlock) {
        // read and clear in one atomic: a kernel of another stream may be adding
        v += atomicExch(&slots[i * kSegStride], 0ull);
    }
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0u) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < kBlock / 64u; ++w) t += part[w];
        if (t) atomicAdd(counter, t);
    }
}

// Sums (and clears) the work counters of the segment slots (kinds 1..) into
// out[kind] (counting launches).
__global__ __launch_bounds__(kBlock) void work_collect_kernel(unsigned long long* __restrict__ slots,
                                                              unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[WO_WORK_KINDS][kBlock / 64];
    static_assert(kSegSlots == kBlock, "one slot per thread");
    const uint32_t i = threadIdx.x;
#pragma unroll
    for (uint32_t k = 1; k < WO_WORK_KINDS; ++k) {
        unsigned long long v = slots[i * kSegStride + k];
        slots[i * kSegStride + k] = 0ull;
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((i & 63u) == 0u) part[k][i >> 6] = v;
    }
    __syncthreads();
    if (i > 0u && i < WO_WORK_KINDS) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < kBlock / 64u; ++w) t += part[i][w];
        out[i] = t;
    }
}

__global__ __launch_bounds__(kBlock) void assemble_kernel(const float4* __restrict__ gathered, float4* __restrict__ frame,
                                                          uint32_t W, uint32_t H, uint32_t T, uint32_t N,
                                                          uint32_t cycle, uint32_t skip, uint32_t local_rows) {
    size_t total = (size_t)W * H;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        uint32_t y = (uint32_t)(i / W), x = (uint32_t)(i - (size_t)y * W);
        uint32_t g = y / T;
        uint32_t r, lb;
        band_local(g, N, cycle, skip, r, lb);
        uint32_t lrow = lb * T + (y - g * T);
        frame[i] = gathered[((size_t)r * local_rows + lrow) * W + x];
    }
}

// Present encode (present.c): float RGBA -> B8G8R8A8 sRGB, the reference's
// preferred swapchain format (renderer.c:813-832).  A channel's code is the
// count of the 255 thresholds <= its value (binary search in LDS), which is
// round-half-up(255 * srgb(clamp(v))) exactly; NaN -> 0.  HBM-bound: 16 B read
// + 4 B written per pixel.
__device__ __forceinline__ uint32_t srgb8_code(const float* t, float v) {
    uint32_t k = 0;
#pragma unroll
    for (uint32_t s = 128u; s > 0u; s >>= 1)
        if (t[k + s - 1u] <= v) k += s;  // t[255] = +inf keeps k <= 255
    return k;
}
__device__ __forceinline__ uint32_t unorm8(float a) {
    if (!(a > 0.0f)) return 0u;
    if (a >= 1.0f) return 255u;
    return (uint32_t)((double)a * 255.0 + 0.5);  // exact in double: round-half-up
}
__global__ __launch_bounds__(kBlock) void srgb8_kernel(const float4* __restrict__ in, uint32_t* __restrict__ out,
                                                       size_t n, const float* __restrict__ tab) {
    __shared__ float t[256];
    t[threadIdx.x] = threadIdx.x < 255u ? tab[threadIdx.x] : kInf;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) {
        const float4 p = in[i];
        out[i] = srgb8_code(t, p.z) | (srgb8_code(t, p.y) << 8) | (srgb8_code(t, p.x) << 16) | (unorm8(p.w) << 24);
    }
}

// Exhaustive check of sqrt_cr / rcp_cr over float bit patterns [lo, lo + count)
// against the definition of correct rounding, evaluated exactly in double
// (independent of any library expansion): s = RN(sqrt x) iff (s - u/2)^2 <= x
// <= (s + u/2)^2, u = ulp(s) (the squares of 25-bit numbers are exact in double,
// and no float x sits on a midpoint); r = RN(1/x) iff |1 - r x| <= (u/2) |x|,
// u = ulp(r) (r x is exact in double).  Counts the patterns that fail.
__global__ __launch_bounds__(kBlock) void fastmath_check_kernel(uint32_t lo, uint32_t count, int which,
                                                                unsigned long long* __restrict__ bad,
                                                                uint32_t* __restrict__ first_bad) {
    unsigned long long nbad = 0;
    uint32_t first = 0xffffffffu;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock) {
        const uint32_t u = lo + i;
        const float x = __uint_as_float(u);
        bool ok;
        if (which == 0) {
            const float s = sqrt_cr(x);
            const double sd = s, h = 0.5 * ((double)__uint_as_float(__float_as_uint(s) + 1u) - sd);
            ok = (sd - h) * (sd - h) <= (double)x && (double)x <= (sd + h) * (sd + h);
        } else {
            const float r = rcp_cr(x);
            const double rd = r, h = 0.5 * fabs((double)__uint_as_float(__float_as_uint(r) + 1u) - rd);
            ok = fabs(1.0 - rd * (double)x) <= h * fabs((double)x);
        }
        if (!ok) {
            ++nbad;
            first = u < first ? u : first;
        }
    }
    for (int off = 32; off > 0; off >>= 1) nbad += __shfl_xor(nbad, off, 64);
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)first, off, 64);
        first = o < first ? o : first;
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (nbad) atomicAdd(bad, nbad);
        if (first != 0xffffffffu) atomicMin(first_bad, first);
    }
}

}  // namespace

extern "C" int wo_fastmath_check(int which, uint32_t lo_bits, uint32_t hi_bits, unsigned long long* mismatches,
                                 uint32_t* first_mismatch) {
    unsigned long long* d_bad = nullptr;
    uint32_t* d_first = nullptr;
    if (hi_bits < lo_bits) return -1;
    if (hipMalloc((void**)&d_bad, sizeof *d_bad) != hipSuccess) return -1;
    if (hipMalloc((void**)&d_first, sizeof *d_first) != hipSuccess) {
        (void)hipFree(d_bad);
        return -1;
    }
    const uint32_t init = 0xffffffffu;
    hipError_t e = hipMemset(d_bad, 0, sizeof *d_bad);
    if (e == hipSuccess) e = hipMemcpy(d_first, &init, sizeof init, hipMemcpyHostToDevice);
    const uint64_t total = (uint64_t)hi_bits - lo_bits + 1u;
    for (uint64_t done = 0; e == hipSuccess && done < total;) {
        const uint32_t n = (uint32_t)(total - done < (1ull << 30) ? total - done : (1ull << 30));
        hipLaunchKernelGGL(fastmath_check_kernel, dim3(8192), dim3(kBlock), 0, nullptr, (uint32_t)(lo_bits + done), n,
                           which, d_bad, d_first);
        e = hipGetLastError();
        done += n;
    }
    if (e == hipSuccess) e = hipMemcpy(mismatches, d_bad, sizeof *d_bad, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(first_mismatch, d_first, sizeof *d_first, hipMemcpyDeviceToHost);
    (void)hipFree(d_bad);
    (void)hipFree(d_first);
    return e == hipSuccess ? 0 : -1;
}

// ===========================================================================
// Host glue (C ABI declared in wo_dev.h)
// ===========================================================================
// big tiles per resident workgroup of a rank's share (plan_tiles), every kernel;
// a generated source may name its own (`// wo_share_tiles N`, scene_jit.c)
constexpr uint32_t kShareTiles = 3u;

struct WoDev {
    int device;
    int cus;           // compute units (multiProcessorCount)
    std::string arch;  // gcnArchName, e.g. gfx950:sramecc+:xnack-
    WoRec* d_prog;
    size_t prog_cap;
    WoMaterial* d_mats;
    size_t mats_cap;
    uint32_t n_recs, n_prims, n_mats;
    float4* d_frame;
    size_t frame_cap;
    hipStream_t stream;
    // lane tracer: ordinal -> program pc (generic primitives, hit leaves)
    uint32_t* d_ordpc;
    size_t ordpc_cap;
    // the lane tracer's ordered BVH: the builder's blob and its descriptor (lane_bvh.h)
    float4* d_lbvh;
    size_t lbvh_cap;
    WoLaneBvhDesc lbvh;
    uint32_t last_kind;   // the PathKind of the last path launch (wo_dev_lanes_info)
    // ray queries (wo_dev_trace_rays): per program record its source node handle, the
    // host form's staging buffer (rays, then hits), and the last ray launch's kernel
    uint32_t* d_nodes;
    size_t nodes_cap;
    uint32_t n_nodes;
    float4* d_rayio;
    size_t rayio_cap;
    uint32_t ray_kind;     // its PathKind (kLanesBvh / kLanesBvhSpheres / kInterpLds / kInterpGlobal; 0: none yet)
    bool ray_last;         // the last path or ray launch was a ray launch (wo_dev_lanes_info's form)
    unsigned long long* d_segslots;  // kSegSlots segment counters, kSegStride apart
    unsigned long long* d_work;      // WO_WORK_KINDS totals of a counting launch
    // progressive accumulation (3 int64 per pixel) and the frame slots (wo_dev.h
    // WO_SLOT_*): the draw_frame pipeline's two, the synchronous render's scratch
    // slot and the two device-frame slots; a present slot holds a device frame, a
    // pinned host copy and an event
    long long* d_accum;
    size_t accum_cap;
    float4* d_slot[WO_SLOTS];
    size_t dslot_cap[WO_SLOTS];
    float* h_slot[WO_SLOTS];
    size_t hslot_cap[WO_SLOTS];
    uint32_t* d_bgra[WO_SLOTS];  // the slot's frame encoded for present (B8G8R8A8 sRGB)
    size_t dbgra_cap[WO_SLOTS];
    uint32_t* h_bgra[WO_SLOTS];
    size_t hbgra_cap[WO_SLOTS];
    hipEvent_t slot_ev[WO_SLOTS];  // the slot's map-back is done (on copy_stream)
    // Map-back of presented frames: the present encode and
    // the D2H copies run on their own stream, gated by rend_ev (the slot's frame is
    // rendered), so the next frame's kernel starts as soon as this one ends.
    hipStream_t copy_stream;
    // On-demand float map-back of a presented frame (wo_dev_frame_map_float): its own
    // stream, created on first use, so it never queues behind the next frame's
    // map-back on copy_stream (which waits for that frame's render).
    hipStream_t map_stream;
    hipEvent_t rend_ev[WO_SLOTS];
    bool slot_float[WO_SLOTS];  // the float frame was copied with the last map-back
    size_t slot_pixels[WO_SLOTS];  // pixels of the slot's last frame
    bool slot_recorded[WO_SLOTS];  // slot_ev has been recorded (never wait on an unrecorded event)
    // pipeline timestamps (wo_dev_set_stamps): render begin / render end / map-back end
    bool stamps;
    hipEvent_t st_base;
    hipEvent_t st_ev[WO_SLOTS][3];
    bool st_valid[WO_SLOTS];
    // several devices per renderer (wo_dev_frame_submit_ranks): on the root,
    // the rank-major buffer the ranks' shares are copied into and the event that
    // opens a slot to the ranks; on every rank, its share of the frame and the
    // event that marks the share delivered (copied, or staged in host memory)
    float4* d_gather[WO_SLOTS];
    size_t dgather_cap[WO_SLOTS];
    hipEvent_t gate_ev[WO_SLOTS];
    float4* d_part[WO_SLOTS];
    size_t dpart_cap[WO_SLOTS];
    float4* h_part[WO_SLOTS];  // WO_PEER_STAGED: the share's pinned host copy
    size_t hpart_cap[WO_SLOTS];
    hipEvent_t part_ev[WO_SLOTS];
    // the split present (present_rows): this rank's rows encoded for present, and the
    // events that order its encode after its render (psrc), the gather's reuse of
    // the share after the encode (penc) and the root's slot after the D2H (pmap)
    uint32_t* d_pbgra[WO_SLOTS];
    size_t dpbgra_cap[WO_SLOTS];
    hipEvent_t psrc_ev[WO_SLOTS], penc_ev[WO_SLOTS], pmap_ev[WO_SLOTS];
    int peer_mode;  // how this rank's share reaches the root (WO_PEER_*; wo_dev_enable_peer)
    unsigned long long* d_segacc;  // segments of this rank's device frames (wo_dev_take_segments)
    bool lanes_on;
    // scene-specialised kernel (its code object: jit_code.cpp)
    hipModule_t jit_module;
    hipFunction_t jit_fn;
    uint32_t jit_share_tiles;  // big tiles per resident workgroup for the specialised kernel (plan_tiles)
    std::string jit_key;  // SHA-256 (hex) of the loaded code object's inputs
    std::string jit_src;  // its source (the counting variant is built from it on demand)
    hipModule_t count_module;
    hipFunction_t count_fn;
    int jit_attr[3];  // the loaded specialised kernel's scratch bytes per lane, VGPRs, static LDS (kernel_info)
    int jit_origin;       // 0 process cache, 1 disk cache, 2 compiled
    double jit_compile_sec;
};

static void set_err(char* err, size_t len, const char* what, hipError_t e) {
    if (err && len) snprintf(err, len, "%s: %s", what, hipGetErrorString(e));
}

// Zero device memory and wait for it: hipMemset may still be running on the null
// stream when a kernel on one of the non-blocking streams starts, and a late
// memset would wipe what that kernel counted.  (One-time set-ups only.)
static hipError_t zero_now(void* p, size_t bytes) {
    hipError_t e = hipMemset(p, 0, bytes);
    return e == hipSuccess ? hipDeviceSynchronize() : e;
}

extern "C" int wo_hip_runtime_version(void) {
    int v = 0;
    return hipRuntimeGetVersion(&v) == hipSuccess ? v : -1;
}

extern "C" int wo_dev_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int wo_dev_device(WoDev* dev) { return dev ? dev->device : -1; }

extern "C" int wo_dev_select(int device) { return hipSetDevice(device) == hipSuccess ? 0 : -1; }

extern "C" int wo_dev_current(void) {
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess) return -1;
    return d;
}

extern "C" int wo_dev_create(int device, WoDev** out, char* err, size_t errlen) {
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipGetDeviceProperties", e);
        return -1;
    }
    WoDev* dev = new (std::nothrow) WoDev();
    if (!dev) {
        snprintf(err, errlen, "out of host memory");
        return -1;
    }
    dev->device = device;
    dev->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
    dev->arch = prop.gcnArchName;
    e = hipStreamCreateWithFlags(&dev->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipStreamCreate", e);
        delete dev;
        return -1;
    }
    e = hipStreamCreateWithFlags(&dev->copy_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipStreamCreate(copy)", e);
        (void)hipStreamDestroy(dev->stream);
        delete dev;
        return -1;
    }
    *out = dev;
    return 0;
}

extern "C" void wo_dev_destroy(WoDev* dev) {
    if (!dev) return;
    (void)hipSetDevice(dev->device);
    // device frames assemble on the caller's stream from this rank's buffers
    (void)hipDeviceSynchronize();
    if (dev->d_prog) (void)hipFree(dev->d_prog);
    if (dev->d_mats) (void)hipFree(dev->d_mats);
    if (dev->d_frame) (void)hipFree(dev->d_frame);
    if (dev->d_lbvh) (void)hipFree(dev->d_lbvh);
    if (dev->d_ordpc) (void)hipFree(dev->d_ordpc);
    if (dev->d_nodes) (void)hipFree(dev->d_nodes);
    if (dev->d_rayio) (void)hipFree(dev->d_rayio);
    if (dev->d_segslots) (void)hipFree(dev->d_segslots);
    if (dev->d_work) (void)hipFree(dev->d_work);
    if (dev->d_accum) (void)hipFree(dev->d_accum);
    if (dev->d_segacc) (void)hipFree(dev->d_segacc);
    for (int i = 0; i < WO_SLOTS; ++i) {
        if (dev->h_part[i]) (void)hipHostFree(dev->h_part[i]);
        if (dev->d_slot[i]) (void)hipFree(dev->d_slot[i]);
        if (dev->h_slot[i]) (void)hipHostFree(dev->h_slot[i]);
        if (dev->slot_ev[i]) (void)hipEventDestroy(dev->slot_ev[i]);
        if (dev->d_bgra[i]) (void)hipFree(dev->d_bgra[i]);
        if (dev->h_bgra[i]) (void)hipHostFree(dev->h_bgra[i]);
        if (dev->d_gather[i]) (void)hipFree(dev->d_gather[i]);
        if (dev->gate_ev[i]) (void)hipEventDestroy(dev->gate_ev[i]);
        if (dev->d_part[i]) (void)hipFree(dev->d_part[i]);
        if (dev->part_ev[i]) (void)hipEventDestroy(dev->part_ev[i]);
        if (dev->d_pbgra[i]) (void)hipFree(dev->d_pbgra[i]);
        for (hipEvent_t ev : {dev->psrc_ev[i], dev->penc_ev[i], dev->pmap_ev[i]})
            if (ev) (void)hipEventDestroy(ev);
        if (dev->rend_ev[i]) (void)hipEventDestroy(dev->rend_ev[i]);
        for (int k = 0; k < 3; ++k)
            if (dev->st_ev[i][k]) (void)hipEventDestroy(dev->st_ev[i][k]);
    }
    if (dev->st_base) (void)hipEventDestroy(dev->st_base);
    if (dev->jit_module) (void)hipModuleUnload(dev->jit_module);
    if (dev->count_module) (void)hipModuleUnload(dev->count_module);
    if (dev->map_stream) (void)hipStreamDestroy(dev->map_stream);
    (void)hipStreamDestroy(dev->copy_stream);
    (void)hipStreamDestroy(dev->stream);
    delete dev;
}

template <class T>
static int ensure_buffer(T** p, size_t* cap, size_t bytes, char* err, size_t errlen) {
    if (bytes <= *cap && *p) return 0;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    size_t alloc = bytes ? bytes : 64;
    hipError_t e = hipMalloc((void**)p, alloc);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipMalloc", e);
        return -1;
    }
    *cap = alloc;
    return 0;
}

// The kernels' view of the lane BVH (built on the host, lane_bvh_build.cpp): the
// blob's sections through the descriptor's offsets.
static LaneBvh lane_bvh(const WoDev* dev) {
    const WoLaneBvhDesc& d = dev->lbvh;
    const uint32_t* words = reinterpret_cast<const uint32_t*>(dev->d_lbvh);
    LaneBvh b;
    b.nodes = dev->d_lbvh;
    b.geo = dev->d_lbvh + lane_node_f4(d) * d.nodes;
    b.kind = reinterpret_cast<const uint32_t*>(b.geo + d.nprims);
    b.nalways = d.always;
    b.root = d.root;
    b.nprims = d.nprims;
    b.ntop = d.top;
    b.depth = d.depth;
    // csg512_balanced: 60.4 / 57.6 / 57.2 / 58.1 / 59.2 ms at 8 / 16 / 24 / 32 / 40;
    // WOLOLO_DYN_WALKERS (measurement) overrides
    static const uint32_t walkers = [] {
        const char* w = getenv("WOLOLO_DYN_WALKERS");
        return w && *w ? (uint32_t)atoi(w) : 24u;
    }();
    b.dyn_walkers = walkers;
    b.trec = d.terms ? reinterpret_cast<const float4*>(words + d.term_off) : nullptr;
    b.leaves = d.leaf_off ? reinterpret_cast<const WoRec*>(words + d.leaf_off) : nullptr;
    b.gpar = words + d.gpar_off;
    b.gnode = words + d.gnode_off;
    b.gclip = d.gclip_off ? reinterpret_cast<const float4*>(words + d.gclip_off) : nullptr;
    b.gP = d.gP;
    b.gwords = d.gwords;
    b.groot = d.groot;
    return b;
}

template <class T>
static int upload(T** p, size_t* cap, const void* src, size_t bytes, const char* what, char* err, size_t errlen) {
    if (ensure_buffer(p, cap, bytes, err, errlen)) return -1;
    const hipError_t e = bytes ? hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
    if (e != hipSuccess) {
        set_err(err, errlen, what, e);
        return -1;
    }
    return 0;
}

extern "C" int wo_dev_upload_scene(WoDev* dev, WoRec const* prog, uint32_t n_recs, uint32_t n_prims,
                                   WoMaterial const* mats, uint32_t n_mats, char* err, size_t errlen) {
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    // Kernels of the previous scene may still run on any stream of the device
    // (the frame pipeline's, or a caller's stream for render_rows_device): the
    // buffers below are overwritten (or reallocated) in place and the JIT module
    // replaced next, so the whole device drains first.  Scene changes are rare.
    e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        set_err(err, errlen, "hipDeviceSynchronize (before scene upload)", e);
        return -1;
    }
    if (upload(&dev->d_prog, &dev->prog_cap, prog, (size_t)n_recs * sizeof(WoRec), "hipMemcpy(program)", err, errlen))
        return -1;
    if (upload(&dev->d_mats, &dev->mats_cap, mats, (size_t)n_mats * sizeof(WoMaterial), "hipMemcpy(materials)", err,
               errlen))
        return -1;
    dev->n_recs = n_recs;
    dev->n_prims = n_prims;
    dev->n_mats = n_mats;
    dev->n_nodes = ~0u;  // the node table is the previous scene's until wo_dev_upload_nodes
    LaneBvhBuild lb;
    if (lane_bvh_build(prog, n_recs, n_prims, mats, n_mats, &lb, err, errlen)) return -1;
    dev->lbvh = lb.desc;
    if (upload(&dev->d_ordpc, &dev->ordpc_cap, lb.ordpc.data(), lb.ordpc.size() * sizeof(uint32_t),
               "hipMemcpy(ordinal map)", err, errlen))
        return -1;
    // (no lane form: no blob, and no kernel that reads d_lbvh is launched)
    return lb.blob.empty() ? 0
                           : upload(&dev->d_lbvh, &dev->lbvh_cap, lb.blob.data(), lb.blob.size(), "hipMemcpy(lane BVH)",
                                    err, errlen);
}

// ---- scene-specialised kernels: their code objects are jit_code.cpp's; loaded here ----

static int load_jit_module(const std::vector<char>& code, hipModule_t* mod, hipFunction_t* fn, char* err,
                           size_t errlen) {
    hipError_t e = hipModuleLoadData(mod, code.data());
    if (e != hipSuccess) {
        set_err(err, errlen, "hipModuleLoadData", e);
        return -1;
    }
    e = hipModuleGetFunction(fn, *mod, "wo_jit_pathtrace");
    if (e != hipSuccess) {
        (void)hipModuleUnload(*mod);
        *mod = nullptr;
        set_err(err, errlen, "hipModuleGetFunction", e);
        return -1;
    }
    return 0;
}

extern "C" int wo_dev_set_jit(WoDev* dev, const char* src, char* err, size_t errlen) {
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    if (dev->count_module) (void)hipModuleUnload(dev->count_module);  // built again on demand
    dev->count_module = nullptr;
    dev->count_fn = nullptr;
    if (!src) {  // disable
        if (dev->jit_module) (void)hipModuleUnload(dev->jit_module);
        dev->jit_module = nullptr;
        dev->jit_fn = nullptr;
        dev->jit_key.clear();
        dev->jit_src.clear();
        dev->jit_origin = -1;
        return 0;
    }
    wojit::JitCode jc;
    if (dev->jit_fn && dev->jit_key == wojit::jit_key(src, dev->arch)) return 0;
    if (wojit::jit_code(src, dev->arch, false, &jc, err, errlen)) return -1;
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    if (load_jit_module(jc.code, &mod, &fn, err, errlen)) return -1;
    if (dev->jit_module) (void)hipModuleUnload(dev->jit_module);
    dev->jit_module = mod;
    dev->jit_fn = fn;
    dev->jit_key = jc.key;
    // its resources, read now: once the counting variant (the same kernel name in another
    // module) is loaded, an attribute query of this function returned that one's scratch
    // size -- and a second renderer's counting module can do the same at load time, so
    // the scratch and LDS sizes come from this code object's kernel descriptor
    dev->jit_attr[0] = dev->jit_attr[1] = dev->jit_attr[2] = -1;
    (void)hipFuncGetAttribute(&dev->jit_attr[0], HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, fn);
    (void)hipFuncGetAttribute(&dev->jit_attr[1], HIP_FUNC_ATTRIBUTE_NUM_REGS, fn);
    (void)hipFuncGetAttribute(&dev->jit_attr[2], HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, fn);
    {
        uint32_t group = 0, priv = 0;
        if (wojit::kd_segment_sizes(jc.code.data(), jc.code.size(), "wo_jit_pathtrace", &group, &priv)) {
            dev->jit_attr[0] = (int)priv;
            dev->jit_attr[2] = (int)group;
        }
    }
    dev->jit_src = src;
    {
        const char* m = strstr(src, "// wo_share_tiles ");
        const int v = m ? atoi(m + strlen("// wo_share_tiles ")) : 0;
        dev->jit_share_tiles = v >= 1 && v <= 64 ? (uint32_t)v : kShareTiles;
    }
    dev->jit_origin = jc.origin;
    dev->jit_compile_sec = jc.seconds;
    return 0;
}

extern "C" int wo_dev_jit_cached(WoDev* dev, const char* src) {
    std::vector<char> code;
    return wojit::jit_lookup(wojit::jit_key(src, dev->arch), &code) >= 0 ? 1 : 0;
}

extern "C" WoJitJob* wo_jit_job_start(WoDev* dev, const char* src) { return wojit::jit_job_start(src, dev->arch); }

extern "C" int wo_dev_jit_origin(WoDev* dev, double* seconds) {
    if (!dev || !dev->jit_fn) return -1;
    if (seconds) *seconds = dev->jit_compile_sec;
    return dev->jit_origin;
}

extern "C" int wo_dev_lanes_info(WoDev* dev, uint32_t* out) {
    if (!dev) return -1;
    out[0] = dev->lbvh.nodes;
    out[1] = dev->lbvh.depth;
    out[2] = dev->lbvh.top;
    out[3] = dev->lbvh.always;
    out[4] = dev->ray_last ? dev->ray_kind : dev->last_kind;
    return 0;
}

extern "C" int wo_dev_jit_active(WoDev* dev) { return dev && dev->jit_fn ? 1 : 0; }
static bool has_lane_form(const WoLaneBvhDesc& d) { return d.union_only || d.terms || d.general; }
extern "C" int wo_dev_lanes_available(WoDev* dev) { return dev && has_lane_form(dev->lbvh) ? 1 : 0; }
extern "C" void wo_dev_set_lanes(WoDev* dev, int on) {
    if (dev) dev->lanes_on = on != 0;
}
extern "C" double wo_dev_jit_compile_sec(WoDev* dev) { return dev ? dev->jit_compile_sec : 0.0; }

// Path-tracer launch grid (PathLaunch): big tiles first, then a tail of small
// 4x4 tiles sized to ~3 waves of resident workgroups, which fills the end of
// the frame while the last big tiles finish.  Measured (csg32 1080p64, slowest
// rank, tools/rank_share.py): no tail 5.57 / 2.87 / 1.60 / 1.09 ms at N = 1 / 2 /
// 4 / 8 (8x8 tiles throughout); 3-round tail 5.50 / 2.81 / 1.53 / 0.81 ms.  The big shape is 8x8
// while the frame holds >= 8 rounds of such tiles, else 8x4 (2-round tail), else 4x4
// (plan_tiles); `resident` = workgroups the device holds at once.  Env (measurements):
// WOLOLO_TILE=8x8|8x4|4x4 forces one shape everywhere, with no tail.
// "WxH" with W, H in {1, 2, 4, 8, 16} and W*H <= kTileMaxPix; 0 if not such a shape
static uint32_t shape_of(const char* f) {
    unsigned w = 0, h = 0;
    if (sscanf(f, "%ux%u", &w, &h) != 2) return 0u;
    auto lg = [](unsigned v) -> int { return v == 1u ? 0 : v == 2u ? 1 : v == 4u ? 2 : v == 8u ? 3 : v == 16u ? 4 : -1; };
    const int lw = lg(w), lh = lg(h);
    if (lw < 0 || lh < 0 || w * h > kTileMaxPix) return 0u;
    return (uint32_t)lw | ((uint32_t)lh << 4);
}
static uint32_t tiles_across(uint32_t width, uint32_t shape) { return (width + (1u << (shape & 15u)) - 1u) >> (shape & 15u); }

// *n_wg: the workgroups to launch, the big tiles and the small ones over the rows left
static PathLaunch plan_tiles(uint32_t width, uint32_t rows, uint32_t resident, uint32_t band_rows,
                             uint32_t want_per_wg, uint64_t* n_wg) {
    const uint32_t s44 = 2u | (2u << 4);
    PathLaunch g = {};
    // the tail's tiles: 4x4 (2x2 / 4x2 for an 8-rank share's tail: within noise,
    // DESIGN.md §6)
    const uint32_t small = s44;
    g.small_log2 = small;
    g.tiles_x_small = tiles_across(width, small);
    const uint32_t sh = 1u << (small >> 4);
    double tail_rounds = 3.0;  // rounds of resident workgroups in the tail
    const char* f = getenv("WOLOLO_TILE");  // a forced tile shape ("8x4"): the whole frame in it
    uint32_t big = (f && *f) ? shape_of(f) : 0u;
    if (big) {
        tail_rounds = 0.0;
    } else {
        // The largest shape that gives every resident workgroup >= want_per_wg tiles
        // (kShareTiles = 3 for every kernel since round 5, see the end of this note): a
        // workgroup's tiles then average out the costly ones (glass, deep CSG),
        // which otherwise set the end of a short launch.  8x8 keeps a 3-round
        // tail of 4x4 tiles, 8x4 a 2-round one.  Measured (tools/rank_share.py,
        // 1080p64, slowest rank of 4 / 8, ms): csg32 8x8 1.454 / 0.770, 8x4 1.400 /
        // 0.762, 4x4 1.499 / 0.786; csg256 balanced 8x4 4.73 / 3.50, 4x4 4.23 / 2.34;
        // csg256 chain 8x4 7.34 / 5.02, 4x4 7.99 / 4.15; rtiow 8x4 8.47 / 4.30,
        // 4x4 8.27 / 4.37.  One GPU keeps 8x8 (csg32 5.18 vs 5.37 ms at 8x4).  Round 4
        // (tools/root_step.py, N = 8 projection): 3 tiles per resident workgroup instead
        // of 8 (8x4 at N = 8): csg32 6.37 -> 6.62x, csg256 balanced 6.79 -> 4.18x,
        // chain 6.83 -> 4.75x, csg32_nested 6.35 -> 5.83x, RTIOW 6.59 -> 6.63x; kept at 8.
        // Round 5 (camera-ray waves, tools/root_step.py at N = 8 without the present
        // map-back, band 5:1): small tiles now cost more -- a wave drains its last paths
        // at the end of every tile, and a 4x4 tile gives a wave 4 camera iterations (the
        // whole csg32 frame in 4x4 tiles: 2.77 -> 3.33 ms) -- so the specialised kernels
        // of trees up to depth 32 (the generator's `wo_share_tiles`) want 3 tiles per
        // resident workgroup: csg32 6.30 -> 6.87x, csg32_nested 7.09 -> 7.66x, csg256
        // balanced 6.88 -> 7.19x; the chain keeps 8 (6.96 -> 6.46x with 3: its costly tiles
        // set the end of a share); the lane tracer keeps 8.  Those runs put rank 0's five
        // streams on HIP's 4 hardware queues, so a render could queue behind a copy; with
        // bench.py's layout (two render streams + one gather stream, 8 queues) 3 wins for
        // every scene (want 3 / 8, N = 8 projection): csg32 6.86 / 6.40x, csg32_nested
        // 7.67 / 7.27x, balanced 7.17 / 6.78x, chain 6.99 / 6.88x, RTIOW 7.37 / 6.97x,
        // csg512 6.00 / 5.45x, C4 7.59 / 7.60x (profiles/r05_root_step_want_hwq8.log).
        // So every kernel passes kShareTiles (the lane tracer, the interpreter and a
        // specialised kernel without the generator's marker included).
        const char* tw = getenv("WOLOLO_TILE_WANT");  // (measurement) tiles per resident workgroup
        const char* ts = getenv("WOLOLO_TILE_SPAN");  // (measurement) 8x8 tiles may span two row bands
        const uint64_t want_tiles = (uint64_t)(tw && *tw ? (uint32_t)atoi(tw) : want_per_wg) * resident;
        const bool span = ts && *ts == '1';
        big = 3u | (3u << 4);
        if ((uint64_t)tiles_across(width, big) * (rows >> 3) < want_tiles || (band_rows < 8u && !span)) {
            big = 3u | (2u << 4);
            tail_rounds = 2.0;
        }
        if ((uint64_t)tiles_across(width, big) * (rows >> 2) < want_tiles) big = s44;
    }
    g.big_log2 = big;
    g.tiles_x_big = tiles_across(width, big);
    const uint32_t bh = 1u << (big >> 4);
    uint32_t rows_small = 0;
    if (tail_rounds > 0.0 && big != small) {
        uint64_t want = (uint64_t)(tail_rounds * resident + 0.5);
        rows_small = (uint32_t)(((want + g.tiles_x_small - 1u) / g.tiles_x_small) * sh);
    }
    uint32_t rows_big = rows > rows_small ? ((rows - rows_small) / bh) * bh : 0u;
    if (big == small) rows_big = ((rows + bh - 1u) / bh) * bh;  // one shape: the big grid covers everything
    g.rows_big = rows_big;
    g.n_big = g.tiles_x_big * (rows_big / bh);
    *n_wg = g.n_big + (rows > rows_big ? (uint64_t)g.tiles_x_small * ((rows - rows_big + sh - 1u) / sh) : 0u);
    return g;
}

// The planner without a device (CPU tests): out = big_log2, small_log2, n_big,
// tiles_x_big, tiles_x_small, rows_big, workgroups; -1 where launch_impl refuses the frame.
extern "C" int wo_plan_tiles(uint32_t width, uint32_t rows, uint32_t resident, uint32_t band_rows,
                             uint32_t want_per_wg, uint32_t out[7]) {
    uint64_t n_wg = 0;
    const PathLaunch g = plan_tiles(width, rows, resident, band_rows, want_per_wg, &n_wg);
    const uint32_t v[7] = {g.big_log2, g.small_log2, g.n_big, g.tiles_x_big, g.tiles_x_small, g.rows_big, (uint32_t)n_wg};
    memcpy(out, v, sizeof v);
    return n_wg < (1ull << 31) ? 0 : -1;
}

static const size_t kLdsBudget = 64u * 1024u;

extern "C" int wo_dev_launch(WoDev* dev, WoFrame const* frame_in, void* d_out, void* stream_v,
                             unsigned long long* d_segments, char* err, size_t errlen) {
    return wo_dev_launch_ex(dev, frame_in, d_out, stream_v, d_segments, nullptr, 0u, err, errlen);
}

// the numbers are wo_renderer_lanes_info's "kind" (the lane tracer's forms, LaneTracer)
enum PathKind { kLanesBvh = 2, kLanesBvhSpheres = 3, kLanesTerms = 6, kLanesGeneral = 7, kLanesDynWideTerms = 14,
                kJit = 16, kInterpLds = 17, kInterpGlobal = 18 };

// The library's kernel of a kind (`count`: its counting variant) for the pointer
// forms of the occupancy, attribute and launch calls; nullptr for kJit, whose
// kernel is the device's loaded module.  The lane kernels take lane_args' list,
// the interpreter's interp_args'.
template <bool kCount>
static const void* path_kernel_of(PathKind kind) {
    switch (kind) {
    case kLanesBvh: return (const void*)pathtrace_lanes_kernel<2, kCount>;
    case kLanesBvhSpheres: return (const void*)pathtrace_lanes_kernel<3, kCount>;
    case kLanesTerms: return (const void*)pathtrace_lanes_kernel<6, kCount>;
    case kLanesGeneral: return (const void*)pathtrace_lanes_kernel<7, kCount>;
    case kLanesDynWideTerms: return (const void*)pathtrace_lanes_kernel<14, kCount>;
    case kInterpLds: return (const void*)pathtrace_kernel<true, kCount>;
    case kInterpGlobal: return (const void*)pathtrace_kernel<false, kCount>;
    case kJit: break;
    }
    return nullptr;
}
static const void* path_kernel(PathKind kind, bool count) {
    return !count ? path_kernel_of<false>(kind) : path_kernel_of<true>(kind);
}
// the same for a ray launch's four kernels
static const void* ray_kernel(PathKind kind) {
    switch (kind) {
    case kLanesBvh: return (const void*)trace_rays_lanes_kernel<2>;
    case kLanesBvhSpheres: return (const void*)trace_rays_lanes_kernel<3>;
    case kInterpLds: return (const void*)trace_rays_kernel<true>;
    case kInterpGlobal: return (const void*)trace_rays_kernel<false>;
    default: return nullptr;
    }
}
// a feature launch's kernel: the ray kernels' forms, each for 8 x 8 tiles or 64 x 1 strips
template <bool kTile>
static const void* feature_kernel_of(PathKind kind) {
    switch (kind) {
    case kLanesBvh: return (const void*)features_lanes_kernel<2, kTile>;
    case kLanesBvhSpheres: return (const void*)features_lanes_kernel<3, kTile>;
    case kInterpLds: return (const void*)features_kernel<true, kTile>;
    case kInterpGlobal: return (const void*)features_kernel<false, kTile>;
    default: return nullptr;
    }
}
static const void* feature_kernel(PathKind kind, bool tile) {
    return tile ? feature_kernel_of<true>(kind) : feature_kernel_of<false>(kind);
}
// a span launch's kernel: the program in LDS or not, the sweep's window 4, 8 or 16 keys wide
template <bool kProgInLds>
static const void* span_kernel_of(int window) {
    switch (window) {
    case 4: return (const void*)trace_spans_kernel<kProgInLds, 4>;
    case 8: return (const void*)trace_spans_kernel<kProgInLds, 8>;
    default: return (const void*)trace_spans_kernel<kProgInLds, 16>;
    }
}
static const void* span_kernel(PathKind kind, int window) {
    return kind == kInterpLds ? span_kernel_of<true>(window) : span_kernel_of<false>(window);
}
// a mass launch's kernel: the program in LDS or not, the window, the wave's footprint, the accumulators' home
template <bool kProgInLds, int kN, bool kTile>
static const void* mass_kernel_red(int red) {
    switch (red) {
    case kMassShfl: return (const void*)mass_grid_kernel<kProgInLds, kN, kTile, kMassShfl>;
    case kMassLds: return (const void*)mass_grid_kernel<kProgInLds, kN, kTile, kMassLds>;
    default: return (const void*)mass_grid_kernel<kProgInLds, kN, kTile, kMassRegs>;
    }
}
template <bool kProgInLds>
static const void* mass_kernel_of(int window, bool tile, int red) {
    if (window == 8) return tile ? mass_kernel_red<kProgInLds, 8, true>(red) : mass_kernel_red<kProgInLds, 8, false>(red);
    return tile ? mass_kernel_red<kProgInLds, 16, true>(red) : mass_kernel_red<kProgInLds, 16, false>(red);
}
static const void* mass_kernel(PathKind kind, int window, bool tile, int red) {
    return kind == kInterpLds ? mass_kernel_of<true>(window, tile, red) : mass_kernel_of<false>(window, tile, red);
}
static bool is_lane_kind(PathKind kind) { return kind < kJit; }

// The path kernel of the last launch: key_hex (65 bytes) gets the specialised
// kernel's code-object key (jit_key) or "static:<kind>:<source hash>"; out[0] = kind (PathKind),
// out[1] = private bytes per lane, out[2] = registers (VGPRs), out[3] = static LDS
// bytes.  A profile session records these beside its counters, so a summary says
// which code object it measured.
static int kernel_info_current(WoDev* dev, char* key_hex, uint32_t* out) {  // dev's device is current
    const PathKind kind = (PathKind)dev->last_kind;
    out[0] = (uint32_t)kind;
    if (kind == kJit) {
        if (!dev->jit_fn || dev->jit_attr[0] < 0 || dev->jit_attr[1] < 0 || dev->jit_attr[2] < 0) return -1;
        out[1] = (uint32_t)dev->jit_attr[0];  // read when the module was loaded (wo_dev_set_jit)
        out[2] = (uint32_t)dev->jit_attr[1];
        out[3] = (uint32_t)dev->jit_attr[2];
        if (key_hex) snprintf(key_hex, 65, "%s", dev->jit_key.c_str());
    } else {
        // "static:<kind>:" + the first 40 hex digits of the library kernels' source hash
        hipFuncAttributes a;
        if (hipFuncGetAttributes(&a, path_kernel(kind, false)) != hipSuccess) return -1;
        out[1] = (uint32_t)a.localSizeBytes;
        out[2] = (uint32_t)a.numRegs;
        out[3] = (uint32_t)a.sharedSizeBytes;
        if (key_hex) snprintf(key_hex, 65, "static:%u:%.40s", (unsigned)kind, WO_STATIC_SRC_SHA);
    }
    return 0;
}

// (the caller's current device is restored on every path, as renderer.c's multi-device entries do)
extern "C" int wo_dev_kernel_info(WoDev* dev, char* key_hex, uint32_t* out) {
    if (!dev || !out || dev->last_kind == 0u) return -1;
    const int prev = wo_dev_current();
    if (hipSetDevice(dev->device) != hipSuccess) return -1;
    const int rc = kernel_info_current(dev, key_hex, out);
    if (prev >= 0) (void)hipSetDevice(prev);
    return rc;
}

static int launch_impl(WoDev* dev, WoFrame const* frame_in, void* d_out, void* stream_v,
                       unsigned long long* d_segments, long long* d_accum, uint32_t accum_spp, bool count, char* err,
                       size_t errlen);

// The interpreter's per-wave LDS scratch (KLayout) for a program of n_recs records
// and n_prims primitives, and its form: the program in LDS too when both fit
// (kInterpLds), else read from global memory (kInterpGlobal).  The frame kernel
// and the ray kernel share it.
static int interp_plan(uint32_t n_recs, uint32_t n_prims, KLayout* lay, PathKind* kind, size_t* dyn_lds, char* err,
                       size_t errlen) {
    lay->codes_words = (n_recs + 7u) / 8u + 1u;
    lay->ordpc_off = lay->codes_words;
    uint32_t hib_words = n_prims > 64u ? (n_prims - 64u + 31u) / 32u : 0u;
    lay->hib_off = lay->ordpc_off + n_prims;
    lay->wave_words = (lay->hib_off + hib_words * 64u + 3u) & ~3u;
    size_t scratch = (size_t)(kBlock / 64u) * lay->wave_words * 4u;
    size_t prog_bytes = (size_t)n_recs * sizeof(WoRec);
    if (prog_bytes + scratch <= kLdsBudget) {
        *kind = kInterpLds;
        *dyn_lds = prog_bytes + scratch;
    } else if (scratch <= kLdsBudget) {
        *kind = kInterpGlobal;
        *dyn_lds = scratch;
    } else {
        snprintf(err, errlen, "scene too large for the LDS scratch (%zu bytes per workgroup)", scratch);
        return -1;
    }
    return 0;
}

extern "C" int wo_dev_launch_ex(WoDev* dev, WoFrame const* frame_in, void* d_out, void* stream_v,
                                unsigned long long* d_segments, long long* d_accum, uint32_t accum_spp, char* err,
                                size_t errlen) {
    return launch_impl(dev, frame_in, d_out, stream_v, d_segments, d_accum, accum_spp, false, err, errlen);
}

// `count`: the counting variant of the chosen path kernel (work counters in the
// segment slots; wo_dev_count_work collects them).
static int launch_impl(WoDev* dev, WoFrame const* frame_in, void* d_out, void* stream_v,
                       unsigned long long* d_segments, long long* d_accum, uint32_t accum_spp, bool count, char* err,
                       size_t errlen) {
    hipStream_t stream = (hipStream_t)stream_v;  // NULL = the null stream (HIP convention)
    WoFrame fr = *frame_in;
    if (fr.width == 0 || fr.height == 0) return 0;
    if (fr.tile_rows == 0 || fr.nranks == 0 || fr.rank >= fr.nranks) {
        snprintf(err, errlen, "bad row tiling (tile_rows=%u rank=%u nranks=%u)", fr.tile_rows, fr.rank, fr.nranks);
        return -1;
    }
    if (fr.n_recs != dev->n_recs || fr.n_prims != dev->n_prims) {
        snprintf(err, errlen, "frame/scene mismatch (recs %u vs %u)", fr.n_recs, dev->n_recs);
        return -1;
    }
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    uint32_t local_rows = wo_rank_local_rows_ex(fr.height, fr.tile_rows, fr.nranks, fr.band_cycle, fr.band_skip);
    float4* out = (float4*)d_out;

    if (fr.mode == WO_MODE_UBERSHADER_RT1 || fr.mode == WO_MODE_DEBUG_ST) {
        dim3 grid((fr.width + kBlock - 1) / kBlock, local_rows);
        hipLaunchKernelGGL(ubershader_kernel, grid, dim3(kBlock), 0, stream, fr, local_rows, out);
    } else if (fr.mode == WO_MODE_PATHTRACE || fr.mode == WO_MODE_NORMALS) {
        if (fr.n_prims >= (1u << 20)) {
            snprintf(err, errlen, "scene has %u primitives (max %u)", fr.n_prims, (1u << 20) - 1u);
            return -1;
        }
        // the kernels count segments into the per-device slots; seg_collect_kernel
        // then moves the sum into the caller's counter
        unsigned long long* slots = nullptr;
        if (d_segments) {
            if (!dev->d_segslots) {
                e = hipMalloc((void**)&dev->d_segslots, kSegSlots * kSegStride * sizeof(unsigned long long));
                if (e == hipSuccess)
                    e = zero_now(dev->d_segslots, kSegSlots * kSegStride * sizeof(unsigned long long));
                if (e != hipSuccess) {
                    dev->d_segslots = nullptr;
                    set_err(err, errlen, "hipMalloc(segment slots)", e);
                    return -1;
                }
            }
            slots = dev->d_segslots;
        }
        // which kernel, with how much dynamic LDS; then the workgroups one CU holds
        PathKind kind;
        size_t dyn_lds = 0;
        KLayout lay = {};
        const WoLaneBvhDesc& lb = dev->lbvh;
        if (dev->lanes_on && has_lane_form(lb) && !dev->jit_fn) {
            // the ordered BVH, its lane stacks and top nodes in LDS; the 4-wide tree (term mode
            // over more than 256 terms) runs the resumable walk
            kind = lb.wide      ? kLanesDynWideTerms
                   : lb.terms   ? kLanesTerms
                   : lb.general ? kLanesGeneral
                   : (lb.spheres_only ? kLanesBvhSpheres : kLanesBvh);
            dyn_lds = lane_bvh_lds(lb);
        } else if (dev->jit_fn) {
            kind = kJit;
        } else if (interp_plan(fr.n_recs, fr.n_prims, &lay, &kind, &dyn_lds, err, errlen)) {
            return -1;
        }
        dev->last_kind = (uint32_t)kind;
        dev->ray_last = false;
        int per_cu = 0;
        hipFunction_t jfn = count ? dev->count_fn : dev->jit_fn;
        if (kind == kJit)
            e = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, jfn, kBlock, 0);
        else
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, path_kernel(kind, count), kBlock, dyn_lds);
        if (e != hipSuccess || per_cu < 1) per_cu = 1;
        // a rank's local rows are bands of tile_rows consecutive frame rows: a tile
        // taller than a band would join rows far apart (incoherent primary rays)
        uint64_t n_wg = 0;
        PathLaunch tg = plan_tiles(fr.width, local_rows, (uint32_t)dev->cus * (uint32_t)per_cu,
                                   fr.nranks > 1u ? fr.tile_rows : ~0u, kind == kJit ? dev->jit_share_tiles : kShareTiles,
                                   &n_wg);
        if (d_accum && fr.mode == WO_MODE_PATHTRACE) {
            tg.acc = d_accum;
            tg.acc_spp = accum_spp;
        }
        if (n_wg >= (1ull << 31)) {
            snprintf(err, errlen, "frame too large (%llu workgroups)", (unsigned long long)n_wg);
            return -1;
        }
        dim3 grid((uint32_t)n_wg);
        if (kind == kJit) {
            const WoRec* p = dev->d_prog;
            const WoMaterial* m = dev->d_mats;
            unsigned long long* sl = slots;
            PathLaunch plv = tg;
            void* args[] = {&p, &m, &fr, &local_rows, &out, &sl, &plv};
            e = hipModuleLaunchKernel(jfn, grid.x, 1, 1, kBlock, 1, 1, 0, stream, args, nullptr);
            if (e != hipSuccess) {
                set_err(err, errlen, "hipModuleLaunchKernel", e);
                return -1;
            }
        } else {
            LaneBvh bvh = lane_bvh(dev);
            void* lane_args[] = {&dev->d_prog, &dev->d_ordpc, &dev->d_mats, &fr, &local_rows, &out, &slots, &tg, &bvh};
            void* interp_args[] = {&dev->d_prog, &dev->d_mats, &fr, &lay, &local_rows, &out, &slots, &tg};
            // (a failed launch is hipGetLastError's below)
            (void)hipLaunchKernel(path_kernel(kind, count), grid, dim3(kBlock), is_lane_kind(kind) ? lane_args : interp_args,
                                  dyn_lds, stream);
        }
        if (slots) hipLaunchKernelGGL(seg_collect_kernel, dim3(1), dim3(kBlock), 0, stream, slots, d_segments);
    } else {
        snprintf(err, errlen, "unknown shading mode %u", fr.mode);
        return -1;
    }
    e = hipGetLastError();
    if (e != hipSuccess) {
        set_err(err, errlen, "kernel launch", e);
        return -1;
    }
    return 0;
}

// ---- ray queries ----

extern "C" int wo_dev_upload_nodes(WoDev* dev, uint32_t const* nodes, uint32_t n_recs, char* err, size_t errlen) {
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    dev->n_nodes = ~0u;
    if (upload(&dev->d_nodes, &dev->nodes_cap, nodes, (size_t)n_recs * sizeof(uint32_t), "hipMemcpy(node table)", err,
               errlen))
        return -1;
    dev->n_nodes = n_recs;
    return 0;
}

extern "C" int wo_dev_ray_form(WoDev* dev) {
    if (!dev || dev->ray_kind == 0u) return 0;
    return dev->ray_kind == kLanesBvh || dev->ray_kind == kLanesBvhSpheres ? 2 : 1;
}

// Workgroups of a ray launch: one ray per lane, at most the workgroups the device
// holds at once (the grid-stride loop takes the rest).  WOLOLO_RAY_BLOCKS
// (measurement) caps the grid.
static uint32_t ray_grid(const WoDev* dev, size_t n, int per_cu) {
    uint64_t blocks = ((uint64_t)n + kBlock - 1u) / kBlock;
    uint64_t resident = (uint64_t)dev->cus * (uint64_t)(per_cu < 1 ? 1 : per_cu);
    const char* cap = getenv("WOLOLO_RAY_BLOCKS");
    if (cap && *cap && atoi(cap) > 0) resident = (uint64_t)atoi(cap);
    return (uint32_t)(blocks < resident ? blocks : resident);
}

extern "C" int wo_dev_trace_rays(WoDev* dev, void const* d_rays, void* d_hits, size_t n, int form, void* stream_v,
                                 char* err, size_t errlen) {
    hipStream_t stream = (hipStream_t)stream_v;  // NULL = the null stream (HIP convention)
    if (n == 0) return 0;
    if (!dev->d_prog || !dev->d_nodes || dev->n_nodes != dev->n_recs) {
        snprintf(err, errlen, "no scene (or no node table) on the device");
        return -1;
    }
    if (((uintptr_t)d_rays | (uintptr_t)d_hits) & 15u) {
        snprintf(err, errlen, "ray and hit buffers must be 16-byte aligned");
        return -1;
    }
    if (dev->n_prims >= (1u << 20)) {
        snprintf(err, errlen, "scene has %u primitives (max %u)", dev->n_prims, (1u << 20) - 1u);
        return -1;
    }
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    RayBatch rb;
    rb.rays = (const float4*)d_rays;
    rb.hits = (float4*)d_hits;
    rb.nodes = dev->d_nodes;
    rb.n = n;
    rb.n_mats = dev->n_mats;
    // the lane walk for a union-only scene (its BVH is built at every upload), unless
    // the interpreter is asked for; a scene that is not union-only has no plain walk
    const WoLaneBvhDesc& lb = dev->lbvh;
    const bool lanes = form != 1 && lb.union_only && !lb.stack16;  // (the ray kernels' stacks are 32-bit)
    PathKind kind;
    size_t dyn_lds = 0;
    KLayout lay = {};
    if (lanes) {
        kind = lb.spheres_only ? kLanesBvhSpheres : kLanesBvh;
        dyn_lds = lane_bvh_lds(lb);
    } else if (interp_plan(dev->n_recs, dev->n_prims, &lay, &kind, &dyn_lds, err, errlen)) {
        return -1;
    }
    const void* kernel = ray_kernel(kind);
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, dyn_lds);
    if (e != hipSuccess || per_cu < 1) per_cu = 1;
    LaneBvh bvh = lane_bvh(dev);
    void* lane_args[] = {&dev->d_prog, &dev->d_ordpc, &bvh, &rb};
    void* interp_args[] = {&dev->d_prog, &dev->n_recs, &lay, &rb};
    (void)hipLaunchKernel(kernel, dim3(ray_grid(dev, n, per_cu)), dim3(kBlock), lanes ? lane_args : interp_args, dyn_lds,
                          stream);
    e = hipGetLastError();
    if (e != hipSuccess) {
        set_err(err, errlen, "ray kernel launch", e);
        return -1;
    }
    dev->ray_kind = (uint32_t)kind;
    dev->ray_last = true;
    return 0;
}

extern "C" int wo_dev_trace_rays_host(WoDev* dev, void const* rays, void* hits, size_t n, int form, char* err,
                                      size_t errlen) {
    if (n == 0) return 0;
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    const size_t bytes = n * 2u * sizeof(float4);  // rays, and as many bytes of hits behind them
    if (ensure_buffer(&dev->d_rayio, &dev->rayio_cap, 2u * bytes, err, errlen)) return -1;
    float4* d_rays = dev->d_rayio;
    float4* d_hits = dev->d_rayio + 2u * n;
    e = hipMemcpyAsync(d_rays, rays, bytes, hipMemcpyHostToDevice, dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipMemcpy(rays)", e);
        return -1;
    }
    if (wo_dev_trace_rays(dev, d_rays, d_hits, n, form, dev->stream, err, errlen)) return -1;
    e = hipMemcpyAsync(hits, d_hits, bytes, hipMemcpyDeviceToHost, dev->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "ray query", e);
        return -1;
    }
    return 0;
}

// ---- first-hit feature buffers ----

// The wave's footprint (DESIGN 3.12 holds the measurement; the planes do not depend on
// it): WOLOLO_FEATURE_TILE = 8x8 | 64x1.
static bool feature_tile() {
    const char* v = getenv("WOLOLO_FEATURE_TILE");
    return !(v && strcmp(v, "64x1") == 0);
}

extern "C" int wo_dev_features(WoDev* dev, WoFrame const* frame, void* d_out, size_t plane_stride, int form,
                               void* stream_v, char* err, size_t errlen) {
    hipStream_t stream = (hipStream_t)stream_v;  // NULL = the null stream (HIP convention)
    if (!dev->d_prog || !dev->d_nodes || dev->n_nodes != dev->n_recs) {
        snprintf(err, errlen, "no scene (or no node table) on the device");
        return -1;
    }
    FeatureLaunch fl;
    fl.fr = *frame;
    if (fl.fr.width == 0 || fl.fr.height == 0 || fl.fr.spp == 0 || fl.fr.tile_rows == 0 || fl.fr.nranks == 0 ||
        fl.fr.rank >= fl.fr.nranks) {
        snprintf(err, errlen, "bad frame (%ux%u, spp=%u, tile_rows=%u rank=%u nranks=%u)", fl.fr.width, fl.fr.height,
                 fl.fr.spp, fl.fr.tile_rows, fl.fr.rank, fl.fr.nranks);
        return -1;
    }
    if (fl.fr.n_recs != dev->n_recs || fl.fr.n_prims != dev->n_prims) {
        snprintf(err, errlen, "frame/scene mismatch (recs %u vs %u)", fl.fr.n_recs, dev->n_recs);
        return -1;
    }
    fl.local_rows = wo_rank_local_rows_ex(fl.fr.height, fl.fr.tile_rows, fl.fr.nranks, fl.fr.band_cycle, fl.fr.band_skip);
    if (!d_out || ((uintptr_t)d_out & 15u) || plane_stride < (size_t)fl.local_rows * fl.fr.width) {
        snprintf(err, errlen, "the planes' buffer must be device memory, 16-byte aligned, plane_stride >= %zu rows",
                 (size_t)fl.local_rows * fl.fr.width);
        return -1;
    }
    if (dev->n_prims >= (1u << 20)) {
        snprintf(err, errlen, "scene has %u primitives (max %u)", dev->n_prims, (1u << 20) - 1u);
        return -1;
    }
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    fl.mats = dev->d_mats;
    fl.nodes = dev->d_nodes;
    fl.out = (uint4*)d_out;
    fl.plane_stride = plane_stride;
    fl.n_mats = dev->n_mats;
    // the kernel family of the ray queries (wo_dev_trace_rays)
    const WoLaneBvhDesc& lb = dev->lbvh;
    const bool lanes = form != 1 && lb.union_only && !lb.stack16;
    PathKind kind;
    size_t dyn_lds = 0;
    KLayout lay = {};
    if (lanes) {
        kind = lb.spheres_only ? kLanesBvhSpheres : kLanesBvh;
        dyn_lds = lane_bvh_lds(lb);
    } else if (interp_plan(dev->n_recs, dev->n_prims, &lay, &kind, &dyn_lds, err, errlen)) {
        return -1;
    }
    const bool tile = feature_tile();
    const void* kernel = feature_kernel(kind, tile);
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, dyn_lds);
    if (e != hipSuccess || per_cu < 1) per_cu = 1;
    // one item (tile or strip) per wave: ray_grid's count for as many lanes
    const uint64_t items = tile ? (uint64_t)((fl.fr.width + 7u) / 8u) * ((fl.local_rows + 7u) / 8u)
                                : (uint64_t)((fl.fr.width + 63u) / 64u) * fl.local_rows;
    LaneBvh bvh = lane_bvh(dev);
    void* lane_args[] = {&dev->d_prog, &dev->d_ordpc, &bvh, &fl};
    void* interp_args[] = {&dev->d_prog, &dev->n_recs, &lay, &fl};
    (void)hipLaunchKernel(kernel, dim3(ray_grid(dev, (size_t)(items * 64u), per_cu)), dim3(kBlock),
                          lanes ? lane_args : interp_args, dyn_lds, stream);
    e = hipGetLastError();
    if (e != hipSuccess) {
        set_err(err, errlen, "feature kernel launch", e);
        return -1;
    }
    dev->ray_kind = (uint32_t)kind;
    dev->ray_last = true;
    return 0;
}

extern "C" int wo_dev_features_host(WoDev* dev, WoFrame const* frame, void* out, int form, char* err, size_t errlen) {
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    const size_t pixels = (size_t)frame->width * frame->height, bytes = 3u * pixels * sizeof(float4);
    if (ensure_buffer(&dev->d_rayio, &dev->rayio_cap, bytes, err, errlen)) return -1;
    if (wo_dev_features(dev, frame, dev->d_rayio, pixels, form, dev->stream, err, errlen)) return -1;
    e = hipMemcpyAsync(out, dev->d_rayio, bytes, hipMemcpyDeviceToHost, dev->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "feature query", e);
        return -1;
    }
    return 0;
}

// ---- ray span queries and point classification ----

// The span sweep's window (SpanWindow): 16 keys, one re-collect pass per 16 events
// (1080p batches, tools/ray_span_bench.py, window 4 / 8 / 16: csg32_nested pixel rays
// 0.461 / 0.403 / 0.358 ms, through rays csg256_chain 3.22 / 3.22 / 2.86 and rtiow_cover
// 1.28 / 1.15 / 1.12; csg32 pixel rays, one or two events each, 0.113 / 0.118 / 0.121).
// WOLOLO_SPAN_WINDOW = 4 | 8 | 16 (measurement) picks another; the results do not
// depend on it.
static int span_window() {
    const char* w = getenv("WOLOLO_SPAN_WINDOW");
    const int v = w && *w ? atoi(w) : 16;
    return v == 4 || v == 8 ? v : 16;
}

extern "C" int wo_dev_trace_spans(WoDev* dev, void const* d_rays, void* d_spans, void* d_crossings, size_t n,
                                  uint32_t max_crossings, void* stream_v, char* err, size_t errlen) {
    hipStream_t stream = (hipStream_t)stream_v;  // NULL = the null stream (HIP convention)
    if (n == 0) return 0;
    if (!dev->d_prog || !dev->d_nodes || dev->n_nodes != dev->n_recs) {
        snprintf(err, errlen, "no scene (or no node table) on the device");
        return -1;
    }
    if (max_crossings != 0u && !d_crossings) {
        snprintf(err, errlen, "NULL crossing buffer with max_crossings = %u", max_crossings);
        return -1;
    }
    if (((uintptr_t)d_rays | (uintptr_t)d_spans | (uintptr_t)d_crossings) & 15u) {
        snprintf(err, errlen, "ray, span and crossing buffers must be 16-byte aligned");
        return -1;
    }
    if (dev->n_prims >= (1u << 20)) {
        snprintf(err, errlen, "scene has %u primitives (max %u)", dev->n_prims, (1u << 20) - 1u);
        return -1;
    }
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    SpanBatch sb;
    sb.rays = (const float4*)d_rays;
    sb.spans = (uint4*)d_spans;
    sb.crossings = max_crossings ? (float4*)d_crossings : nullptr;
    sb.nodes = dev->d_nodes;
    sb.n = n;
    sb.max_crossings = max_crossings;
    PathKind kind;
    size_t dyn_lds = 0;
    KLayout lay = {};
    if (interp_plan(dev->n_recs, dev->n_prims, &lay, &kind, &dyn_lds, err, errlen)) return -1;
    const void* kernel = span_kernel(kind, span_window());
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, dyn_lds);
    if (e != hipSuccess || per_cu < 1) per_cu = 1;
    void* args[] = {&dev->d_prog, &dev->n_recs, &lay, &sb};
    (void)hipLaunchKernel(kernel, dim3(ray_grid(dev, n, per_cu)), dim3(kBlock), args, dyn_lds, stream);
    e = hipGetLastError();
    if (e != hipSuccess) {
        set_err(err, errlen, "span kernel launch", e);
        return -1;
    }
    dev->ray_kind = (uint32_t)kind;
    dev->ray_last = true;
    return 0;
}

extern "C" int wo_dev_trace_spans_host(WoDev* dev, void const* rays, void* spans, void* crossings, size_t n,
                                       uint32_t max_crossings, char* err, size_t errlen) {
    if (n == 0) return 0;
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    // rays (2 rows each), then the summaries (1 row), then the crossings (max_crossings rows)
    const size_t cross_rows = n * (size_t)max_crossings;
    if (ensure_buffer(&dev->d_rayio, &dev->rayio_cap, (3u * n + cross_rows) * sizeof(float4), err, errlen)) return -1;
    float4* d_rays = dev->d_rayio;
    float4* d_spans = d_rays + 2u * n;
    float4* d_cross = d_spans + n;
    e = hipMemcpyAsync(d_rays, rays, 2u * n * sizeof(float4), hipMemcpyHostToDevice, dev->stream);
    // the caller's crossing rows go up first: rows the query does not write come back as they were
    if (e == hipSuccess && cross_rows)
        e = hipMemcpyAsync(d_cross, crossings, cross_rows * sizeof(float4), hipMemcpyHostToDevice, dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipMemcpy(rays)", e);
        return -1;
    }
    if (wo_dev_trace_spans(dev, d_rays, d_spans, cross_rows ? d_cross : nullptr, n, max_crossings, dev->stream, err,
                           errlen))
        return -1;
    e = hipMemcpyAsync(spans, d_spans, n * sizeof(float4), hipMemcpyDeviceToHost, dev->stream);
    if (e == hipSuccess && cross_rows)
        e = hipMemcpyAsync(crossings, d_cross, cross_rows * sizeof(float4), hipMemcpyDeviceToHost, dev->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "span query", e);
        return -1;
    }
    return 0;
}

// ---- mass properties ----

// The mass kernel's form (DESIGN 3.11 holds the measurements; the sums do not depend
// on it): WOLOLO_MASS_TILE = 8x8 | 64x1, WOLOLO_MASS_WINDOW = 8 | 16,
// WOLOLO_MASS_REDUCE = regs | shfl | lds (measurement).
static bool mass_tile() {
    const char* v = getenv("WOLOLO_MASS_TILE");
    return !(v && strcmp(v, "64x1") == 0);
}
static int mass_window() {
    const char* v = getenv("WOLOLO_MASS_WINDOW");
    return v && atoi(v) == 8 ? 8 : 16;
}
static int mass_reduce() {
    const char* v = getenv("WOLOLO_MASS_REDUCE");
    if (v && strcmp(v, "shfl") == 0) return kMassShfl;
    if (v && strcmp(v, "lds") == 0) return kMassLds;
    return kMassRegs;
}
// WOLOLO_MASS_FLUSH = wave (measurement): every wave adds its totals to the sums itself
static uint32_t mass_block_flush() {
    const char* v = getenv("WOLOLO_MASS_FLUSH");
    return v && strcmp(v, "wave") == 0 ? 0u : 1u;
}

extern "C" int wo_dev_mass_sums(WoDev* dev, WoMassLaunch const* ml, void* d_sums, void* stream_v, char* err,
                                size_t errlen) {
    hipStream_t stream = (hipStream_t)stream_v;  // NULL = the null stream (HIP convention)
    if (!dev->d_prog || !dev->d_nodes || dev->n_nodes != dev->n_recs) {
        snprintf(err, errlen, "no scene (or no node table) on the device");
        return -1;
    }
    if (!d_sums || ((uintptr_t)d_sums & 7u)) {
        snprintf(err, errlen, "the sums' buffer must be device memory, 8-byte aligned");
        return -1;
    }
    if (ml->axis > 2u || ml->nu == 0u || ml->nu > 32768u || ml->v_count == 0u || ml->v_count > 32768u ||
        ml->v_begin > 32768u - ml->v_count) {
        snprintf(err, errlen, "bad mass grid");
        return -1;
    }
    if (dev->n_prims >= (1u << 20)) {
        snprintf(err, errlen, "scene has %u primitives (max %u)", dev->n_prims, (1u << 20) - 1u);
        return -1;
    }
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    PathKind kind;
    size_t dyn_lds = 0;
    KLayout lay = {};
    if (interp_plan(dev->n_recs, dev->n_prims, &lay, &kind, &dyn_lds, err, errlen)) return -1;
    if (dyn_lds < kMassReduceLds) dyn_lds = kMassReduceLds;  // the workgroup's reduction reuses the dynamic LDS
    const bool tile = mass_tile();
    const void* kernel = mass_kernel(kind, mass_window(), tile, mass_reduce());
    uint32_t block_flush = mass_block_flush();
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, dyn_lds);
    if (e != hipSuccess || per_cu < 1) per_cu = 1;
    // one item (tile or strip) per wave: ray_grid's count for as many lanes
    const uint64_t items = tile ? (uint64_t)((ml->nu + 7u) / 8u) * ((ml->v_count + 7u) / 8u)
                                : (uint64_t)((ml->nu + 63u) / 64u) * ml->v_count;
    WoMassLaunch launch = *ml;
    unsigned long long* sums = (unsigned long long*)d_sums;
    void* args[] = {&dev->d_prog, &dev->n_recs, &lay, &launch, &sums, &block_flush};
    (void)hipLaunchKernel(kernel, dim3(ray_grid(dev, (size_t)(items * 64u), per_cu)), dim3(kBlock), args, dyn_lds, stream);
    e = hipGetLastError();
    if (e != hipSuccess) {
        set_err(err, errlen, "mass kernel launch", e);
        return -1;
    }
    dev->ray_kind = (uint32_t)kind;
    dev->ray_last = true;
    return 0;
}

extern "C" int wo_dev_mass_sums_host(WoDev* dev, WoMassLaunch const* ml, void* sums, char* err, size_t errlen) {
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    const size_t bytes = 24u * sizeof(unsigned long long);  // Wo_MassSums
    if (ensure_buffer(&dev->d_rayio, &dev->rayio_cap, bytes, err, errlen)) return -1;
    e = hipMemsetAsync(dev->d_rayio, 0, bytes, dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipMemset(sums)", e);
        return -1;
    }
    if (wo_dev_mass_sums(dev, ml, dev->d_rayio, dev->stream, err, errlen)) return -1;
    e = hipMemcpyAsync(sums, dev->d_rayio, bytes, hipMemcpyDeviceToHost, dev->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "mass query", e);
        return -1;
    }
    return 0;
}

extern "C" int wo_dev_classify_points(WoDev* dev, void const* d_points, void* d_out, size_t n, void* stream_v,
                                      char* err, size_t errlen) {
    hipStream_t stream = (hipStream_t)stream_v;  // NULL = the null stream (HIP convention)
    if (n == 0) return 0;
    if (!dev->d_prog) {
        snprintf(err, errlen, "no scene on the device");
        return -1;
    }
    if (((uintptr_t)d_points & 15u) || ((uintptr_t)d_out & 3u)) {
        snprintf(err, errlen, "the point buffer must be 16-byte aligned (the result buffer 4-byte)");
        return -1;
    }
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    // the program in LDS where it fits (the kernel keeps no per-wave scratch)
    const size_t prog_bytes = (size_t)dev->n_recs * sizeof(WoRec);
    const bool in_lds = prog_bytes <= kLdsBudget;
    const size_t dyn_lds = in_lds ? prog_bytes : 0;
    const void* kernel =
        in_lds ? (const void*)classify_points_kernel<true> : (const void*)classify_points_kernel<false>;
    int per_cu = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, dyn_lds);
    if (e != hipSuccess || per_cu < 1) per_cu = 1;
    const float4* pts = (const float4*)d_points;
    uint32_t* out = (uint32_t*)d_out;
    uint64_t n64 = n;
    void* args[] = {&dev->d_prog, &dev->n_recs, &pts, &out, &n64};
    (void)hipLaunchKernel(kernel, dim3(ray_grid(dev, n, per_cu)), dim3(kBlock), args, dyn_lds, stream);
    e = hipGetLastError();
    if (e != hipSuccess) {
        set_err(err, errlen, "point kernel launch", e);
        return -1;
    }
    return 0;
}

extern "C" int wo_dev_classify_points_host(WoDev* dev, void const* points, void* out, size_t n, char* err,
                                           size_t errlen) {
    if (n == 0) return 0;
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    // the points (one row each), then one word per point
    if (ensure_buffer(&dev->d_rayio, &dev->rayio_cap, n * (sizeof(float4) + sizeof(uint32_t)), err, errlen)) return -1;
    float4* d_points = dev->d_rayio;
    uint32_t* d_out = reinterpret_cast<uint32_t*>(d_points + n);
    e = hipMemcpyAsync(d_points, points, n * sizeof(float4), hipMemcpyHostToDevice, dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipMemcpy(points)", e);
        return -1;
    }
    if (wo_dev_classify_points(dev, d_points, d_out, n, dev->stream, err, errlen)) return -1;
    e = hipMemcpyAsync(out, d_out, n * sizeof(uint32_t), hipMemcpyDeviceToHost, dev->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "point query", e);
        return -1;
    }
    return 0;
}

// One frame of this rank with the counting variant of its path kernel:
// counts[WO_WORK_*] are lane counts of what ran (synchronous; the image goes to
// the device's scratch frame and equals the normal kernel's).
extern "C" int wo_dev_count_work(WoDev* dev, WoFrame const* frame, unsigned long long* counts, char* err,
                                 size_t errlen) {
    WoFrame fr = *frame;
    if (fr.mode != WO_MODE_PATHTRACE && fr.mode != WO_MODE_NORMALS) {
        snprintf(err, errlen, "work counters need a path-traced frame");
        return -1;
    }
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    if (dev->jit_fn && !dev->count_fn) {
        wojit::JitCode jc;
        if (wojit::jit_code(dev->jit_src.c_str(), dev->arch, true, &jc, err, errlen)) return -1;
        if (load_jit_module(jc.code, &dev->count_module, &dev->count_fn, err, errlen)) return -1;
    }
    const size_t local_rows = wo_rank_local_rows_ex(fr.height, fr.tile_rows, fr.nranks, fr.band_cycle, fr.band_skip);
    if (ensure_buffer(&dev->d_frame, &dev->frame_cap, local_rows * fr.width * sizeof(float4), err, errlen)) return -1;
    if (!dev->d_work) {
        e = hipMalloc((void**)&dev->d_work, WO_WORK_KINDS * sizeof(unsigned long long));
        if (e != hipSuccess) {
            dev->d_work = nullptr;
            set_err(err, errlen, "hipMalloc(work counters)", e);
            return -1;
        }
    }
    e = hipMemsetAsync(dev->d_work, 0, WO_WORK_KINDS * sizeof(unsigned long long), dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipMemsetAsync(work counters)", e);
        return -1;
    }
    if (launch_impl(dev, &fr, dev->d_frame, dev->stream, dev->d_work, nullptr, 0u, true, err, errlen)) return -1;
    hipLaunchKernelGGL(work_collect_kernel, dim3(1), dim3(kBlock), 0, dev->stream, dev->d_segslots, dev->d_work);
    e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(counts, dev->d_work, WO_WORK_KINDS * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                           dev->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "work counters", e);
        return -1;
    }
    return 0;
}

extern "C" int wo_dev_render_host(WoDev* dev, WoFrame const* frame, float* host_rgba, char* err, size_t errlen) {
    WoFrame fr = *frame;
    fr.tile_rows = 16;
    fr.rank = 0;
    fr.nranks = 1;
    size_t local_rows = wo_rank_local_rows(fr.height, fr.tile_rows, 1);
    size_t bytes = local_rows * fr.width * sizeof(float4);
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    if (ensure_buffer(&dev->d_frame, &dev->frame_cap, bytes, err, errlen)) return -1;
    if (wo_dev_launch(dev, &fr, dev->d_frame, dev->stream, nullptr, err, errlen)) return -1;
    e = hipMemcpyAsync(host_rgba, dev->d_frame, (size_t)fr.width * fr.height * sizeof(float4), hipMemcpyDeviceToHost,
                       dev->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "render (device->host)", e);
        return -1;
    }
    return 0;
}

// ---- progressive accumulation and the draw_frame pipeline (renderer.c) ----

// Frames of the pipeline are whole frames (one rank, 4-row tiles).
static WoFrame whole_frame(WoFrame const* f) {
    WoFrame fr = *f;
    fr.tile_rows = 4;
    fr.rank = 0;
    fr.nranks = 1;
    return fr;
}

extern "C" int wo_dev_accum_prepare(WoDev* dev, uint32_t width, uint32_t height, uint32_t tile_rows,
                                    uint32_t nranks, int reset, long long** d_accum, char* err, size_t errlen) {
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    const size_t bytes = (size_t)width * wo_rank_local_rows(height, tile_rows, nranks) * 3u * sizeof(long long);
    const long long* old = dev->d_accum;
    if (ensure_buffer(&dev->d_accum, &dev->accum_cap, bytes, err, errlen)) return -1;
    if (reset || dev->d_accum != old) {
        e = hipMemsetAsync(dev->d_accum, 0, bytes, dev->stream);
        if (e != hipSuccess) {
            set_err(err, errlen, "hipMemsetAsync(accumulation)", e);
            return -1;
        }
    }
    *d_accum = dev->d_accum;
    return 0;
}

static int ensure_event(hipEvent_t* ev, char* err, size_t errlen) {
    if (*ev) return 0;
    hipError_t e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        *ev = nullptr;
        set_err(err, errlen, "hipEventCreate", e);
        return -1;
    }
    return 0;
}

static int ensure_pinned(void** p, size_t* cap, size_t bytes, char* err, size_t errlen) {
    if (bytes <= *cap && *p) return 0;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t e = hipHostMalloc(p, bytes ? bytes : 64, hipHostMallocDefault);
    if (e != hipSuccess) {
        *p = nullptr;
        set_err(err, errlen, "hipHostMalloc(frame slot)", e);
        return -1;
    }
    *cap = bytes;
    return 0;
}

// The slot's buffers on the device that presents (current device = dev's):
// the device frame (`frame_rows` rows), its pinned host copy, the present
// encode on both sides and the slot event.
static int prep_slot(WoDev* dev, int slot, uint32_t width, uint32_t height, uint32_t frame_rows, char* err,
                     size_t errlen) {
    const size_t pixels = (size_t)width * height;
    if (ensure_buffer(&dev->d_slot[slot], &dev->dslot_cap[slot], (size_t)width * frame_rows * sizeof(float4), err,
                      errlen))
        return -1;
    if (ensure_pinned((void**)&dev->h_slot[slot], &dev->hslot_cap[slot], pixels * sizeof(float4), err, errlen))
        return -1;
    if (ensure_pinned((void**)&dev->h_bgra[slot], &dev->hbgra_cap[slot], pixels * sizeof(uint32_t), err, errlen))
        return -1;
    if (ensure_buffer(&dev->d_bgra[slot], &dev->dbgra_cap[slot], pixels * sizeof(uint32_t), err, errlen)) return -1;
    if (ensure_event(&dev->rend_ev[slot], err, errlen)) return -1;
    return ensure_event(&dev->slot_ev[slot], err, errlen);
}

// Before a frame is rendered into d_slot: the render stream waits for the
// slot's previous map-back (it reads d_slot / d_bgra on the copy stream), and
// the render-begin stamp.
static int open_slot(WoDev* dev, int slot, char* err, size_t errlen) {
    hipError_t e = dev->slot_recorded[slot] ? hipStreamWaitEvent(dev->stream, dev->slot_ev[slot], 0) : hipSuccess;
    if (e == hipSuccess && dev->stamps) e = hipEventRecord(dev->st_ev[slot][0], dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "frame slot gate", e);
        return -1;
    }
    return 0;
}

// After the frame is in d_slot (on the render stream): the map-back on the copy
// stream -- the present encode, its copy to pinned host memory and, when
// `map_float`, the float frame's copy -- then the slot event.  The render stream
// does not wait for any of it: the next frame's kernel starts at once.
// `encoded`: the ranks have already written the present encode into h_bgra (the
// split present, wo_dev_frame_submit_ranks); only the float frame is left.
static int present_slot(WoDev* dev, int slot, size_t pixels, bool map_float, char* err, size_t errlen,
                        bool encoded = false) {
    hipError_t e = dev->stamps ? hipEventRecord(dev->st_ev[slot][1], dev->stream) : hipSuccess;
    if (e == hipSuccess) e = hipEventRecord(dev->rend_ev[slot], dev->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(dev->copy_stream, dev->rend_ev[slot], 0);
    if (e != hipSuccess) {
        set_err(err, errlen, "map-back gate", e);
        return -1;
    }
    dev->slot_float[slot] = map_float || !pixels;
    dev->slot_pixels[slot] = pixels;
    if (pixels) {
        // the present encode (wo_renderer_last_frame_bgra8) and, eagerly or on
        // demand (wo_dev_frame_map_float), the float frame (wo_renderer_last_frame)
        if (!encoded) {
            if (wo_dev_srgb8(dev->d_slot[slot], dev->d_bgra[slot], pixels, dev->copy_stream, err, errlen)) return -1;
            e = hipMemcpyAsync(dev->h_bgra[slot], dev->d_bgra[slot], pixels * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               dev->copy_stream);
        }
        if (e == hipSuccess && map_float)
            e = hipMemcpyAsync(dev->h_slot[slot], dev->d_slot[slot], pixels * sizeof(float4), hipMemcpyDeviceToHost,
                               dev->copy_stream);
        if (e != hipSuccess) {
            set_err(err, errlen, "hipMemcpyAsync(frame slot)", e);
            return -1;
        }
    }
    e = dev->stamps ? hipEventRecord(dev->st_ev[slot][2], dev->copy_stream) : hipSuccess;
    if (e == hipSuccess) e = hipEventRecord(dev->slot_ev[slot], dev->copy_stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipEventRecord", e);
        return -1;
    }
    dev->slot_recorded[slot] = true;
    dev->st_valid[slot] = dev->stamps;
    return 0;
}

static bool present_slot_ok(int slot) { return slot >= 0 && slot <= WO_SLOT_SYNC; }

extern "C" int wo_dev_frame_submit(WoDev* dev, WoFrame const* frame, int slot, long long* d_accum,
                                   uint32_t accum_spp, int map_float, char* err, size_t errlen) {
    if (!present_slot_ok(slot)) {
        snprintf(err, errlen, "bad frame slot %d", slot);
        return -1;
    }
    WoFrame fr = whole_frame(frame);
    hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    if (prep_slot(dev, slot, fr.width, fr.height, wo_rank_local_rows(fr.height, fr.tile_rows, 1u), err, errlen))
        return -1;
    if (open_slot(dev, slot, err, errlen)) return -1;
    if (wo_dev_launch_ex(dev, &fr, dev->d_slot[slot], dev->stream, nullptr, d_accum, accum_spp, err, errlen))
        return -1;
    // whole frame, one rank: the local rows are the frame rows
    return present_slot(dev, slot, (size_t)fr.width * fr.height, map_float != 0, err, errlen);
}

// The float frame of a presented slot whose map-back left it on the device
// (lazy map-back): copied now, synchronously.  The slot must have been waited
// for and not submitted again since.
extern "C" int wo_dev_frame_map_float(WoDev* dev, int slot, float const** host, char* err, size_t errlen) {
    if (!present_slot_ok(slot) || !dev->slot_ev[slot] || !dev->d_slot[slot] || !dev->h_slot[slot]) {
        snprintf(err, errlen, "frame slot %d holds no frame", slot);
        return -1;
    }
    if (!dev->slot_float[slot]) {
        // The presented slot's frame is complete (its slot_ev was waited for when it
        // was presented); the copy runs on map_stream, after slot_ev, so it does not
        // wait for the frame in flight behind it on copy_stream.
        hipError_t e = hipSetDevice(dev->device);
        const size_t bytes = dev->slot_pixels[slot] * sizeof(float4);
        if (e == hipSuccess && !dev->map_stream) e = hipStreamCreateWithFlags(&dev->map_stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamWaitEvent(dev->map_stream, dev->slot_ev[slot], 0);
        if (e == hipSuccess) e = hipMemcpyAsync(dev->h_slot[slot], dev->d_slot[slot], bytes, hipMemcpyDeviceToHost,
                                                dev->map_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(dev->map_stream);
        if (e != hipSuccess) {
            set_err(err, errlen, "float frame map-back", e);
            return -1;
        }
        dev->slot_float[slot] = true;
    }
    *host = dev->h_slot[slot];
    return 0;
}

// Pipeline timestamps: while on, every frame submitted to a present slot records
// three timing events (render begin and end on the render stream, map-back end
// on the copy stream); wo_dev_slot_stamps reads them, in ms after the moment
// stamps were turned on.
extern "C" int wo_dev_set_stamps(WoDev* dev, int on, char* err, size_t errlen) {
    hipError_t e = hipSetDevice(dev->device);
    auto mk = [&](hipEvent_t* ev) {
        if (e == hipSuccess && !*ev) e = hipEventCreate(ev);
    };
    if (on) {
        mk(&dev->st_base);
        for (int i = 0; i < WO_SLOTS; ++i)
            for (int k = 0; k < 3; ++k) mk(&dev->st_ev[i][k]);
        if (e == hipSuccess) e = hipEventRecord(dev->st_base, dev->stream);
    }
    if (e != hipSuccess) {
        set_err(err, errlen, "pipeline stamps", e);
        return -1;
    }
    dev->stamps = on != 0;
    for (int i = 0; i < WO_SLOTS; ++i) dev->st_valid[i] = false;
    return 0;
}

extern "C" int wo_dev_slot_stamps(WoDev* dev, int slot, double out[3]) {
    if (!present_slot_ok(slot) || !dev->st_valid[slot]) return -1;
    for (int k = 0; k < 3; ++k) {
        float ms = 0.0f;
        if (hipEventSynchronize(dev->st_ev[slot][k]) != hipSuccess ||
            hipEventElapsedTime(&ms, dev->st_base, dev->st_ev[slot][k]) != hipSuccess)
            return -1;
        out[k] = ms;
    }
    dev->st_valid[slot] = false;
    return 0;
}

// The caller's view of the device: every stream of it drained (set_devices /
// del before releasing ranks whose buffers the root's streams may still read).
extern "C" int wo_dev_sync(WoDev* dev) {
    if (!dev) return 0;
    return hipSetDevice(dev->device) == hipSuccess && hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

extern "C" int wo_dev_peer_mode(WoDev* dev) { return dev ? dev->peer_mode : -1; }

extern "C" int wo_dev_enable_peer(WoDev* from, WoDev* to, char* err, size_t errlen) {
    const char* pv = getenv("WOLOLO_PEER");
    if (pv && strcmp(pv, "staged") == 0) {
        from->peer_mode = WO_PEER_STAGED;
        return 0;
    }
    if (from->device == to->device) {
        from->peer_mode = WO_PEER_SAME;
        return 0;
    }
    int can = 0;
    hipError_t e = hipDeviceCanAccessPeer(&can, from->device, to->device);
    if (e != hipSuccess || !can) {
        (void)hipGetLastError();
        from->peer_mode = WO_PEER_STAGED;  // no peer path: through pinned host memory
        return 0;
    }
    e = hipSetDevice(from->device);
    if (e == hipSuccess) e = hipDeviceEnablePeerAccess(to->device, 0);
    if (e == hipErrorPeerAccessAlreadyEnabled) {
        (void)hipGetLastError();
        e = hipSuccess;
    }
    if (e != hipSuccess) {
        set_err(err, errlen, "hipDeviceEnablePeerAccess", e);
        return -1;
    }
    from->peer_mode = WO_PEER_DMA;
    return 0;
}

// A frame over n ranks into the root's device buffer `dst`,
// assembled on the root-device stream `s_out`: rank i renders its row-cyclic
// 4-row tiles on its own device and stream once the slot is free (gate: recorded
// on s_out after the slot's previous assembly, so frame k+1 in the other slot
// renders while frame k is still being gathered); ranks 1..n-1 deliver their share into the root's rank-major gather
// buffer (peer DMA over xGMI, a device copy when stacked on the root's device, or
// through pinned host memory without a peer path) and record part_ev; s_out waits
// for every part, then un-interleaves the gathered shares into dst.  The root's
// own share renders on root->stream, straight into its slice of the gather buffer
// (an event orders it when s_out is another stream).  Asynchronous throughout.
// The split present (wo_dev_frame_submit_ranks, WOLOLO_PRESENT_SPLIT=1): rank `rank`
// encodes its own rows for present (srgb8_kernel, the same code per pixel as the
// whole frame's encode) on its copy stream, after its render, and copies them
// straight into the root's pinned frame `h_frame`: its full 4-row bands in one 2D
// copy (band lb is frame band lb * n + rank), a partial last band on its own.  So
// each rank's D2H is 1/n of the frame, over its own link, instead of the root
// copying the whole encoded frame.  Current device: the rank's.
static int present_rows(WoDev* dv, int slot, uint32_t rank, uint32_t n, const WoFrame& fr, const float4* d_rows,
                        hipStream_t src_stream, uint32_t* h_frame, char* err, size_t errlen) {
    const uint32_t T = fr.tile_rows, W = fr.width, H = fr.height;
    const uint32_t lr = wo_rank_local_rows(H, T, n);
    if (ensure_buffer(&dv->d_pbgra[slot], &dv->dpbgra_cap[slot], (size_t)lr * W * sizeof(uint32_t), err, errlen))
        return -1;
    if (ensure_event(&dv->psrc_ev[slot], err, errlen) || ensure_event(&dv->penc_ev[slot], err, errlen) ||
        ensure_event(&dv->pmap_ev[slot], err, errlen))
        return -1;
    const uint32_t cnt = wo_rank_tile_count(H, T, rank, n);
    hipError_t e = hipEventRecord(dv->psrc_ev[slot], src_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(dv->copy_stream, dv->psrc_ev[slot], 0);
    if (e != hipSuccess) {
        set_err(err, errlen, "split present gate", e);
        return -1;
    }
    if (cnt && wo_dev_srgb8(d_rows, dv->d_pbgra[slot], (size_t)cnt * T * W, dv->copy_stream, err, errlen)) return -1;
    e = hipEventRecord(dv->penc_ev[slot], dv->copy_stream);
    if (e == hipSuccess && cnt) {
        const uint32_t g_last = (cnt - 1u) * n + rank;
        const bool partial = (g_last + 1u) * T > H;
        const uint32_t full = cnt - (partial ? 1u : 0u);
        const size_t band = (size_t)T * W * sizeof(uint32_t);
        if (full)
            e = hipMemcpy2DAsync(h_frame + (size_t)rank * T * W, band * n, dv->d_pbgra[slot], band, band, full,
                                 hipMemcpyDeviceToHost, dv->copy_stream);
        if (e == hipSuccess && partial)
            e = hipMemcpyAsync(h_frame + (size_t)g_last * T * W, dv->d_pbgra[slot] + (size_t)(cnt - 1u) * T * W,
                               (size_t)(H - g_last * T) * W * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               dv->copy_stream);
    }
    if (e == hipSuccess) e = hipEventRecord(dv->pmap_ev[slot], dv->copy_stream);
    if (e != hipSuccess) {
        set_err(err, errlen, "split present copy", e);
        return -1;
    }
    return 0;
}

// Off by default: in tools/root_step.py's N = 8 model (csg32, band 2:1) the other
// ranks' shares took 0.447 ms with their encode + D2H against 0.384 without, and
// rank 0's step stayed between 0.30 and 0.55 ms either way (profiles/r06_split_present.log)
static bool present_split_on() {
    static const bool on = [] {
        const char* v = getenv("WOLOLO_PRESENT_SPLIT");
        return v && *v == '1';
    }();
    return on;
}

// `h_present` (the split present): every rank also encodes its rows into the root's
// pinned frame (present_rows); nullptr: the frame is only assembled.
static int ranks_render_assemble(WoDev* const* devs, uint32_t n, WoFrame fr, int slot, long long* const* d_accum,
                                 uint32_t accum_spp, hipStream_t s_out, float4* dst, bool count_segments, char* err,
                                 size_t errlen, uint32_t* h_present = nullptr) {
    WoDev* root = devs[0];
    fr.tile_rows = 4;
    fr.nranks = n;
    fr.band_cycle = fr.band_skip = 0u;  // the C API's device ranks: one band per rank and round
    const uint32_t lr = wo_rank_local_rows(fr.height, fr.tile_rows, n);
    const size_t share = (size_t)lr * fr.width;  // float4s per rank
    hipError_t e = hipSetDevice(root->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    if (ensure_buffer(&root->d_gather[slot], &root->dgather_cap[slot], share * n * sizeof(float4), err, errlen))
        return -1;
    if (!root->gate_ev[slot]) {  // first use of the slot: nothing to wait for beyond what s_out holds
        if (ensure_event(&root->gate_ev[slot], err, errlen)) return -1;
        e = hipEventRecord(root->gate_ev[slot], s_out);
        if (e != hipSuccess) {
            set_err(err, errlen, "hipEventRecord(gate)", e);
            return -1;
        }
    }
    auto seg_counter = [&](WoDev* dv) -> unsigned long long* {
        if (!count_segments) return nullptr;
        if (!dv->d_segacc) {
            hipError_t m = hipMalloc((void**)&dv->d_segacc, sizeof(unsigned long long));
            if (m == hipSuccess) m = zero_now(dv->d_segacc, sizeof(unsigned long long));
            if (m != hipSuccess) {
                dv->d_segacc = nullptr;
                set_err(err, errlen, "hipMalloc(segment counter)", m);
            }
        }
        return dv->d_segacc;
    };
    // rank 0 renders straight into its slice of the gather buffer
    fr.rank = 0;
    unsigned long long* seg0 = seg_counter(root);
    if (count_segments && !seg0) return -1;
    const bool own_stream = s_out != root->stream;
    if (own_stream) {
        if (ensure_event(&root->part_ev[slot], err, errlen)) return -1;
        e = hipStreamWaitEvent(root->stream, root->gate_ev[slot], 0);
        if (e != hipSuccess) {
            set_err(err, errlen, "hipStreamWaitEvent(gate)", e);
            return -1;
        }
    }
    if (wo_dev_launch_ex(root, &fr, root->d_gather[slot], root->stream, seg0, d_accum ? d_accum[0] : nullptr,
                         accum_spp, err, errlen))
        return -1;
    if (h_present && present_rows(root, slot, 0u, n, fr, root->d_gather[slot], root->stream, h_present, err, errlen))
        return -1;
    if (own_stream) {
        e = hipEventRecord(root->part_ev[slot], root->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(s_out, root->part_ev[slot], 0);
        if (e != hipSuccess) {
            set_err(err, errlen, "rank 0 share event", e);
            return -1;
        }
    }
    for (uint32_t i = 1; i < n; ++i) {
        WoDev* dv = devs[i];
        fr.rank = i;
        e = hipSetDevice(dv->device);
        if (e != hipSuccess) {
            set_err(err, errlen, "hipSetDevice", e);
            return -1;
        }
        unsigned long long* seg = seg_counter(dv);
        if (count_segments && !seg) return -1;
        if (ensure_buffer(&dv->d_part[slot], &dv->dpart_cap[slot], share * sizeof(float4), err, errlen)) return -1;
        if (ensure_event(&dv->part_ev[slot], err, errlen)) return -1;
        const bool staged = dv->peer_mode == WO_PEER_STAGED;
        if (staged && ensure_pinned((void**)&dv->h_part[slot], &dv->hpart_cap[slot], share * sizeof(float4), err,
                                    errlen))
            return -1;
        e = hipStreamWaitEvent(dv->stream, root->gate_ev[slot], 0);
        if (e != hipSuccess) {
            set_err(err, errlen, "hipStreamWaitEvent(gate)", e);
            return -1;
        }
        if (wo_dev_launch_ex(dv, &fr, dv->d_part[slot], dv->stream, seg, d_accum ? d_accum[i] : nullptr, accum_spp,
                             err, errlen))
            return -1;
        if (h_present && present_rows(dv, slot, i, n, fr, dv->d_part[slot], dv->stream, h_present, err, errlen))
            return -1;
        float4* slice = root->d_gather[slot] + share * i;
        if (staged)  // device -> pinned host on the rank, host -> root below
            e = hipMemcpyAsync(dv->h_part[slot], dv->d_part[slot], share * sizeof(float4), hipMemcpyDeviceToHost,
                               dv->stream);
        else if (dv->device == root->device)
            e = hipMemcpyAsync(slice, dv->d_part[slot], share * sizeof(float4), hipMemcpyDeviceToDevice, dv->stream);
        else
            e = hipMemcpyPeerAsync(slice, root->device, dv->d_part[slot], dv->device, share * sizeof(float4),
                                   dv->stream);
        if (e == hipSuccess) e = hipEventRecord(dv->part_ev[slot], dv->stream);
        if (e == hipSuccess) e = hipSetDevice(root->device);
        if (e == hipSuccess) e = hipStreamWaitEvent(s_out, dv->part_ev[slot], 0);
        if (e == hipSuccess && staged)
            e = hipMemcpyAsync(slice, dv->h_part[slot], share * sizeof(float4), hipMemcpyHostToDevice, s_out);
        if (e != hipSuccess) {
            set_err(err, errlen, staged ? "gather copy (host-staged)" : "gather copy", e);
            return -1;
        }
    }
    if (wo_dev_assemble(root->d_gather[slot], dst, fr.width, fr.height, fr.tile_rows, n, 0u, 0u, s_out, err, errlen))
        return -1;
    // the slot's buffers are free once the assembly (and the split present's
    // encodes) have read them
    for (uint32_t i = 0; h_present && i < n && e == hipSuccess; ++i) e = hipStreamWaitEvent(s_out, devs[i]->penc_ev[slot], 0);
    if (e == hipSuccess) e = hipEventRecord(root->gate_ev[slot], s_out);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipEventRecord(gate)", e);
        return -1;
    }
    return 0;
}

// The draw_frame pipeline over n ranks: the frame is assembled into the slot's
// device frame on the root's stream and then presented as for one device.
extern "C" int wo_dev_frame_submit_ranks(WoDev* const* devs, uint32_t n, WoFrame const* frame, int slot,
                                         long long* const* d_accum, uint32_t accum_spp, int map_float, char* err,
                                         size_t errlen) {
    if (n <= 1u)
        return wo_dev_frame_submit(devs[0], frame, slot, d_accum ? d_accum[0] : nullptr, accum_spp, map_float, err,
                                   errlen);
    if (!present_slot_ok(slot)) {
        snprintf(err, errlen, "bad frame slot %d", slot);
        return -1;
    }
    WoDev* root = devs[0];
    hipError_t e = hipSetDevice(root->device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    if (prep_slot(root, slot, frame->width, frame->height, frame->height, err, errlen)) return -1;
    if (open_slot(root, slot, err, errlen)) return -1;
    const size_t pixels = (size_t)frame->width * frame->height;
    const bool split = present_split_on() && pixels;
    if (ranks_render_assemble(devs, n, *frame, slot, d_accum, accum_spp, root->stream, root->d_slot[slot], false, err,
                              errlen, split ? root->h_bgra[slot] : nullptr))
        return -1;
    if (!split) return present_slot(root, slot, pixels, map_float != 0, err, errlen);
    // the split present: the encoded frame is already on its way to h_bgra from
    // every rank; the slot's map-back ends when all of those copies have (and the
    // float frame's, when it is mapped eagerly, after the assembly)
    e = hipSetDevice(root->device);
    for (uint32_t i = 0; i < n && e == hipSuccess; ++i) e = hipStreamWaitEvent(root->copy_stream, devs[i]->pmap_ev[slot], 0);
    if (e != hipSuccess) {
        set_err(err, errlen, "split present wait", e);
        return -1;
    }
    return present_slot(root, slot, pixels, map_float != 0, err, errlen, /*encoded=*/true);
}

extern "C" int wo_dev_frame_ranks_device(WoDev* const* devs, uint32_t n, WoFrame const* frame, int slot, void* d_frame,
                                         void* stream, char* err, size_t errlen) {
    if (slot != WO_SLOT_DEV0 && slot != WO_SLOT_DEV1) {
        snprintf(err, errlen, "bad device-frame slot %d", slot);
        return -1;
    }
    if (!d_frame) {
        snprintf(err, errlen, "no device frame");
        return -1;
    }
    WoDev* root = devs[0];
    if (n <= 1u) {  // one rank: straight into the caller's frame (rows >= height are not written)
        WoFrame fr = whole_frame(frame);
        hipError_t e = hipSetDevice(root->device);
        if (e != hipSuccess) {
            set_err(err, errlen, "hipSetDevice", e);
            return -1;
        }
        if (!root->d_segacc) {
            e = hipMalloc((void**)&root->d_segacc, sizeof(unsigned long long));
            if (e == hipSuccess) e = zero_now(root->d_segacc, sizeof(unsigned long long));
            if (e != hipSuccess) {
                root->d_segacc = nullptr;
                set_err(err, errlen, "hipMalloc(segment counter)", e);
                return -1;
            }
        }
        const bool path = fr.mode == WO_MODE_PATHTRACE || fr.mode == WO_MODE_NORMALS;
        return wo_dev_launch(root, &fr, d_frame, stream, path ? root->d_segacc : nullptr, err, errlen);
    }
    const bool path = frame->mode == WO_MODE_PATHTRACE || frame->mode == WO_MODE_NORMALS;
    return ranks_render_assemble(devs, n, *frame, slot, nullptr, 0u, (hipStream_t)stream, (float4*)d_frame, path, err,
                                 errlen);
}

extern "C" int wo_dev_take_segments(WoDev* dev, unsigned long long* total, char* err, size_t errlen) {
    *total = 0;
    if (!dev->d_segacc) return 0;
    hipError_t e = hipSetDevice(dev->device);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(total, dev->d_segacc, sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = zero_now(dev->d_segacc, sizeof(unsigned long long));
    if (e != hipSuccess) {
        set_err(err, errlen, "segment counter", e);
        return -1;
    }
    return 0;
}

extern "C" int wo_dev_frame_wait(WoDev* dev, int slot, float const** host, uint32_t const** host_bgra8, char* err,
                                 size_t errlen) {
    if (!present_slot_ok(slot) || !dev->slot_ev[slot]) {
        snprintf(err, errlen, "frame slot %d was never submitted", slot);
        return -1;
    }
    hipError_t e = hipEventSynchronize(dev->slot_ev[slot]);
    if (e != hipSuccess) {
        set_err(err, errlen, "frame wait", e);
        return -1;
    }
    *host = dev->slot_float[slot] ? dev->h_slot[slot] : nullptr;  // NULL: wo_dev_frame_map_float on demand
    if (host_bgra8) *host_bgra8 = dev->h_bgra[slot];
    return 0;
}

// The present encode's threshold table, one copy per device (built once).
static std::mutex g_srgb_mu;
static float* g_srgb_tab[64];

extern "C" int wo_dev_srgb8(void const* d_rgba, void* d_bgra8, size_t pixels, void* stream, char* err,
                            size_t errlen) {
    if (pixels == 0) return 0;
    int d = -1;
    hipError_t e = hipGetDevice(&d);
    if (e != hipSuccess || d < 0 || d >= 64) {
        set_err(err, errlen, "hipGetDevice", e);
        return -1;
    }
    float* tab = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_srgb_mu);
        if (!g_srgb_tab[d]) {
            float host[255];
            wo_srgb8_thresholds(host);
            float* p = nullptr;
            e = hipMalloc((void**)&p, sizeof host);
            if (e == hipSuccess) e = hipMemcpy(p, host, sizeof host, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                if (p) (void)hipFree(p);
                set_err(err, errlen, "sRGB table upload", e);
                return -1;
            }
            g_srgb_tab[d] = p;
        }
        tab = g_srgb_tab[d];
    }
    size_t blocks = (pixels + kBlock - 1) / kBlock;
    if (blocks > 16384u) blocks = 16384u;
    hipLaunchKernelGGL(srgb8_kernel, dim3((uint32_t)blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)d_rgba, (uint32_t*)d_bgra8, pixels, (const float*)tab);
    e = hipGetLastError();
    if (e != hipSuccess) {
        set_err(err, errlen, "sRGB encode launch", e);
        return -1;
    }
    return 0;
}

extern "C" int wo_dev_assemble(void const* d_gathered, void* d_frame, uint32_t width, uint32_t height,
                               uint32_t tile_rows, uint32_t nranks, uint32_t cycle, uint32_t skip, void* stream,
                               char* err, size_t errlen) {
    if (tile_rows == 0 || nranks == 0) {
        snprintf(err, errlen, "bad tiling");
        return -1;
    }
    uint32_t local_rows = wo_rank_local_rows_ex(height, tile_rows, nranks, cycle, skip);
    size_t total = (size_t)width * height;
    uint32_t blocks = (uint32_t)((total + kBlock - 1) / kBlock);
    if (blocks > 8192u) blocks = 8192u;
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(assemble_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream,
                       (const float4*)d_gathered, (float4*)d_frame, width, height, tile_rows, nranks, cycle, skip,
                       local_rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_err(err, errlen, "assemble launch", e);
        return -1;
    }
    return 0;
}
