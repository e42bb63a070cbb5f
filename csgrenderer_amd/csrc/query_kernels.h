// query_kernels.h -- the library's query kernels for gfx950, device code only: the tracers of
// wo_tracers.h on the caller's rays (trace_rays_*), the frame's first hits (features_*), every
// crossing of a ray (trace_spans_kernel), a grid of rays integrated (mass_grid_kernel), and
// points (classify_points_kernel).  query_launch.hip instantiates and launches them; it
// includes wo_dev.h first (WoMassLaunch, a kernel argument, is declared there).
#pragma once
#include "wo_tracers.h"

namespace {

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

    InterpTracer<false> tr;
    interp_setup<kProgInLds>(tr, smem, gprog, nrec, lay, tid, lane, wave);

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
    WO_LANE_SETUP(tr, prog, ordpc, bvh, smem);
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

    InterpTracer<false> tr;
    interp_setup<kProgInLds>(tr, smem, gprog, nrec, lay, tid, lane, wave);

    const uint32_t W = fl.fr.width, H = fl.fr.height, spp = fl.fr.spp;
    const uint32_t seed_hash = pcg_hash(fl.fr.seed);
    const WaveItems<kTile> items(W, fl.local_rows);
    const uint64_t stride = (uint64_t)gridDim.x * (kBlock / 64u);
    for (uint64_t item = (uint64_t)blockIdx.x * (kBlock / 64u) + wave; item < items.count; item += stride) {
        uint32_t lx, lrow;
        items.cell(item, lane, lx, lrow);
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
// and 3, WO_LANE_SETUP).  Every lane walks on its own, so a lane
// whose pixel is outside the frame does nothing.  Five and six waves per SIMD, not the
// ray kernels' seven and eight: the sums are 15 registers the walk does not have, and
// under the ray kernels' bounds (72 / 64 VGPRs) they spill 72 bytes of scratch per lane.
template <int kMode, bool kTile>
__global__ __launch_bounds__(kBlock, kMode == 2 ? 5 : 6) void features_lanes_kernel(
    const WoRec* __restrict__ prog, const uint32_t* __restrict__ ordpc, LaneBvh bvh, FeatureLaunch fl) {
    static_assert(kMode == 2 || kMode == 3, "feature buffers walk the union-only forms");
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    LaneTracer<kMode, false> tr;
    WO_LANE_SETUP(tr, prog, ordpc, bvh, smem);
    __syncthreads();

    const uint32_t W = fl.fr.width, H = fl.fr.height, spp = fl.fr.spp;
    const uint32_t seed_hash = pcg_hash(fl.fr.seed);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const WaveItems<kTile> items(W, fl.local_rows);
    const uint64_t stride = (uint64_t)gridDim.x * (kBlock / 64u);
    for (uint64_t item = (uint64_t)blockIdx.x * (kBlock / 64u) + wave; item < items.count; item += stride) {
        uint32_t x, lrow;
        items.cell(item, lane, x, lrow);
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

    InterpTracer<false> tr;
    interp_setup<kProgInLds>(tr, smem, gprog, nrec, lay, tid, lane, wave);

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

// kTile: a wave's item is an 8 x 8 tile of cells, else a 64 x 1 strip of one row of the
// row range (WaveItems).
template <bool kProgInLds, int kN, bool kTile, int kRed>
__global__ __launch_bounds__(kBlock) void mass_grid_kernel(const WoRec* __restrict__ gprog, uint32_t nrec, KLayout lay,
                                                           WoMassLaunch ml, unsigned long long* __restrict__ sums,
                                                           uint32_t block_flush) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uni(tid >> 6);

    InterpTracer<false> tr;
    interp_setup<kProgInLds>(tr, smem, gprog, nrec, lay, tid, lane, wave);

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

    const WaveItems<kTile> items(ml.nu, ml.v_count);
    const uint64_t stride = (uint64_t)gridDim.x * (kBlock / 64u);
    for (uint64_t item = (uint64_t)blockIdx.x * (kBlock / 64u) + wave; item < items.count; item += stride) {
        uint32_t ci, cj;
        items.cell(item, lane, ci, cj);
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
    stage_program<kProgInLds>(prog, smem, gprog, nrec, threadIdx.x);
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

}  // namespace
