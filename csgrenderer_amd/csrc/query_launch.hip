// query_launch.hip -- the queries' half of wo_dev.h's C ABI for gfx950 (MI355X, CDNA4, wave64):
// ray queries, first-hit feature buffers, ray spans, mass sums, point classification and the
// surface mesh.  Instantiates the kernels of query_kernels.h and mesh_kernels.h and launches them along one path: the scene
// check, the query's own argument checks, query_plan (which kernel form, how much LDS),
// query_launch (occupancy, grid, launch, record).  The host forms share host_round_trip.
// The queries do not restore the caller's current device.
#include "wo_tracers.h"  // first: every define that shapes device code is made there

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "wo_dev_impl.h"
#include "query_kernels.h"
#include "mesh_kernels.h"

// ---- which kernel: the library's query kernel of a kind, for the pointer forms of the
// occupancy and launch calls ----

// a ray launch's four kernels
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

extern "C" int wo_dev_ray_form(WoDev* dev) {
    if (!dev || dev->ray_kind == 0u) return 0;
    return dev->ray_kind == kLanesBvh || dev->ray_kind == kLanesBvhSpheres ? 2 : 1;
}

// ---- the launch path ----

static int use_device(const WoDev* dev, char* err, size_t errlen) {
    const hipError_t e = hipSetDevice(dev->device);
    if (e != hipSuccess) set_err(err, errlen, "hipSetDevice", e);
    return e == hipSuccess ? 0 : -1;
}

// Every query but the points' reports the node of a leaf: it needs the scene and its node table.
static int scene_check(const WoDev* dev, char* err, size_t errlen) {
    if (dev->d_prog && dev->d_nodes && dev->n_nodes == dev->n_recs) return 0;
    snprintf(err, errlen, "no scene (or no node table) on the device");
    return -1;
}

// A query's kernel form and what a launch of it needs.
struct QueryPlan {
    PathKind kind;
    size_t dyn_lds;
    KLayout lay;  // the interpreter's
    bool lanes;   // the kernel takes the lane kernels' arguments
};

// After the query's own checks: the primitive limit, the device made current, then the lane
// walk for a union-only scene (its BVH is built at every upload) where the query has lane
// kernels (`lane_forms`: rays and features) and the interpreter is not asked for (form 1),
// else the interpreter.  A scene that is not union-only has no plain walk; the plain walk's
// forms (2 and 3) keep 32-bit stacks, so a scene laid out for 16-bit ones is not theirs.
static int query_plan(WoDev* dev, bool lane_forms, int form, QueryPlan* p, char* err, size_t errlen) {
    if (dev->n_prims >= (1u << 20)) {
        snprintf(err, errlen, "scene has %u primitives (max %u)", dev->n_prims, (1u << 20) - 1u);
        return -1;
    }
    if (use_device(dev, err, errlen)) return -1;
    const WoLaneBvhDesc& lb = dev->lbvh;
    *p = {};
    p->lanes = lane_forms && form != 1 && lb.union_only && !lb.stack16;
    if (!p->lanes) return interp_plan(dev->n_recs, dev->n_prims, &p->lay, &p->kind, &p->dyn_lds, err, errlen);
    p->kind = lb.spheres_only ? kLanesBvhSpheres : kLanesBvh;
    p->dyn_lds = lane_bvh_lds(lb);
    return 0;
}

// `kernel` over `lanes` lanes' worth of work with `args`, on at most the workgroups the device
// holds at once (ray_grid).  `what` names the launch in the error text; `record`: the launch
// becomes the device's last ray launch (wo_dev_lanes_info, wo_dev_ray_form).
static int query_launch(WoDev* dev, const void* kernel, size_t dyn_lds, size_t lanes, void** args, hipStream_t stream,
                        const char* what, const PathKind* record, char* err, size_t errlen) {
    int per_cu = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, dyn_lds);
    if (e != hipSuccess || per_cu < 1) per_cu = 1;
    (void)hipLaunchKernel(kernel, dim3(ray_grid(dev, lanes, per_cu)), dim3(kBlock), args, dyn_lds, stream);
    e = hipGetLastError();
    if (e != hipSuccess) {
        set_err(err, errlen, what, e);
        return -1;
    }
    if (record) {
        dev->ray_kind = (uint32_t)*record;
        dev->ray_last = true;
    }
    return 0;
}

// One item (tile or strip) per wave: ray_grid's count for as many lanes.
static size_t item_lanes(bool tile, uint32_t width, uint32_t rows) {
    return (size_t)((tile ? WaveItems<true>(width, rows).count : WaveItems<false>(width, rows).count) * 64u);
}

// A host form's round trip through the device's staging buffer (d_rayio, grown to `bytes`), all
// on the device's own stream: the copies up (a part without a host side is zeroed), `call`
// (the device form, given the buffer), the copies down, then the wait.  A part is `bytes` at
// byte offset `off` of the buffer; empty parts are skipped.
struct IoPart {
    void* host;
    size_t off, bytes;
};
template <class Call>
static int host_round_trip(WoDev* dev, size_t bytes, std::initializer_list<IoPart> up, const char* up_what, Call call,
                           std::initializer_list<IoPart> down, const char* what, char* err, size_t errlen) {
    if (use_device(dev, err, errlen)) return -1;
    if (ensure_buffer(&dev->d_rayio, &dev->rayio_cap, bytes, err, errlen)) return -1;
    char* io = reinterpret_cast<char*>(dev->d_rayio);
    hipError_t e = hipSuccess;
    for (const IoPart& p : up) {
        if (e != hipSuccess || !p.bytes) continue;
        e = p.host ? hipMemcpyAsync(io + p.off, p.host, p.bytes, hipMemcpyHostToDevice, dev->stream)
                   : hipMemsetAsync(io + p.off, 0, p.bytes, dev->stream);
    }
    if (e != hipSuccess) {
        set_err(err, errlen, up_what, e);
        return -1;
    }
    if (call(io)) return -1;
    for (const IoPart& p : down)
        if (e == hipSuccess && p.bytes) e = hipMemcpyAsync(p.host, io + p.off, p.bytes, hipMemcpyDeviceToHost, dev->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dev->stream);
    if (e != hipSuccess) {
        set_err(err, errlen, what, e);
        return -1;
    }
    return 0;
}

// ---- ray queries ----

extern "C" int wo_dev_trace_rays(WoDev* dev, void const* d_rays, void* d_hits, size_t n, int form, void* stream_v,
                                 char* err, size_t errlen) {
    if (n == 0) return 0;
    if (scene_check(dev, err, errlen)) return -1;
    if (((uintptr_t)d_rays | (uintptr_t)d_hits) & 15u) {
        snprintf(err, errlen, "ray and hit buffers must be 16-byte aligned");
        return -1;
    }
    QueryPlan qp;
    if (query_plan(dev, true, form, &qp, err, errlen)) return -1;
    RayBatch rb;
    rb.rays = (const float4*)d_rays;
    rb.hits = (float4*)d_hits;
    rb.nodes = dev->d_nodes;
    rb.n = n;
    rb.n_mats = dev->n_mats;
    LaneBvh bvh = lane_bvh(dev);
    void* lane_args[] = {&dev->d_prog, &dev->d_ordpc, &bvh, &rb};
    void* interp_args[] = {&dev->d_prog, &dev->n_recs, &qp.lay, &rb};
    return query_launch(dev, ray_kernel(qp.kind), qp.dyn_lds, n, qp.lanes ? lane_args : interp_args,
                        (hipStream_t)stream_v, "ray kernel launch", &qp.kind, err, errlen);
}

extern "C" int wo_dev_trace_rays_host(WoDev* dev, void const* rays, void* hits, size_t n, int form, char* err,
                                      size_t errlen) {
    if (n == 0) return 0;
    const size_t bytes = n * 2u * sizeof(float4);  // rays, and as many bytes of hits behind them
    return host_round_trip(
        dev, 2u * bytes, {{const_cast<void*>(rays), 0, bytes}}, "hipMemcpy(rays)",
        [&](char* io) { return wo_dev_trace_rays(dev, io, io + bytes, n, form, dev->stream, err, errlen); },
        {{hits, bytes, bytes}}, "ray query", err, errlen);
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
    if (scene_check(dev, err, errlen)) return -1;
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
    QueryPlan qp;  // the kernel family of the ray queries (wo_dev_trace_rays)
    if (query_plan(dev, true, form, &qp, err, errlen)) return -1;
    fl.mats = dev->d_mats;
    fl.nodes = dev->d_nodes;
    fl.out = (uint4*)d_out;
    fl.plane_stride = plane_stride;
    fl.n_mats = dev->n_mats;
    const bool tile = feature_tile();
    LaneBvh bvh = lane_bvh(dev);
    void* lane_args[] = {&dev->d_prog, &dev->d_ordpc, &bvh, &fl};
    void* interp_args[] = {&dev->d_prog, &dev->n_recs, &qp.lay, &fl};
    return query_launch(dev, feature_kernel(qp.kind, tile), qp.dyn_lds, item_lanes(tile, fl.fr.width, fl.local_rows),
                        qp.lanes ? lane_args : interp_args, (hipStream_t)stream_v, "feature kernel launch", &qp.kind,
                        err, errlen);
}

extern "C" int wo_dev_features_host(WoDev* dev, WoFrame const* frame, void* out, int form, char* err, size_t errlen) {
    const size_t pixels = (size_t)frame->width * frame->height, bytes = 3u * pixels * sizeof(float4);
    return host_round_trip(
        dev, bytes, {}, "",
        [&](char* io) { return wo_dev_features(dev, frame, io, pixels, form, dev->stream, err, errlen); },
        {{out, 0, bytes}}, "feature query", err, errlen);
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
    if (n == 0) return 0;
    if (scene_check(dev, err, errlen)) return -1;
    if (max_crossings != 0u && !d_crossings) {
        snprintf(err, errlen, "NULL crossing buffer with max_crossings = %u", max_crossings);
        return -1;
    }
    if (((uintptr_t)d_rays | (uintptr_t)d_spans | (uintptr_t)d_crossings) & 15u) {
        snprintf(err, errlen, "ray, span and crossing buffers must be 16-byte aligned");
        return -1;
    }
    QueryPlan qp;
    if (query_plan(dev, false, 1, &qp, err, errlen)) return -1;
    SpanBatch sb;
    sb.rays = (const float4*)d_rays;
    sb.spans = (uint4*)d_spans;
    sb.crossings = max_crossings ? (float4*)d_crossings : nullptr;
    sb.nodes = dev->d_nodes;
    sb.n = n;
    sb.max_crossings = max_crossings;
    void* args[] = {&dev->d_prog, &dev->n_recs, &qp.lay, &sb};
    return query_launch(dev, span_kernel(qp.kind, span_window()), qp.dyn_lds, n, args, (hipStream_t)stream_v,
                        "span kernel launch", &qp.kind, err, errlen);
}

extern "C" int wo_dev_trace_spans_host(WoDev* dev, void const* rays, void* spans, void* crossings, size_t n,
                                       uint32_t max_crossings, char* err, size_t errlen) {
    if (n == 0) return 0;
    // rays (2 rows each), then the summaries (1 row), then the crossings (max_crossings rows);
    // the caller's crossing rows go up first: rows the query does not write come back as they were
    const size_t row = sizeof(float4), cross = n * (size_t)max_crossings * row;
    return host_round_trip(
        dev, 3u * n * row + cross, {{const_cast<void*>(rays), 0, 2u * n * row}, {crossings, 3u * n * row, cross}},
        "hipMemcpy(rays)",
        [&](char* io) {
            return wo_dev_trace_spans(dev, io, io + 2u * n * row, cross ? io + 3u * n * row : nullptr, n, max_crossings,
                                      dev->stream, err, errlen);
        },
        {{spans, 2u * n * row, n * row}, {crossings, 3u * n * row, cross}}, "span query", err, errlen);
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
    if (scene_check(dev, err, errlen)) return -1;
    if (!d_sums || ((uintptr_t)d_sums & 7u)) {
        snprintf(err, errlen, "the sums' buffer must be device memory, 8-byte aligned");
        return -1;
    }
    if (ml->axis > 2u || ml->nu == 0u || ml->nu > 32768u || ml->v_count == 0u || ml->v_count > 32768u ||
        ml->v_begin > 32768u - ml->v_count) {
        snprintf(err, errlen, "bad mass grid");
        return -1;
    }
    QueryPlan qp;
    if (query_plan(dev, false, 1, &qp, err, errlen)) return -1;
    if (qp.dyn_lds < kMassReduceLds) qp.dyn_lds = kMassReduceLds;  // the workgroup's reduction reuses the dynamic LDS
    const bool tile = mass_tile();
    uint32_t block_flush = mass_block_flush();
    WoMassLaunch launch = *ml;
    unsigned long long* sums = (unsigned long long*)d_sums;
    void* args[] = {&dev->d_prog, &dev->n_recs, &qp.lay, &launch, &sums, &block_flush};
    return query_launch(dev, mass_kernel(qp.kind, mass_window(), tile, mass_reduce()), qp.dyn_lds,
                        item_lanes(tile, ml->nu, ml->v_count), args, (hipStream_t)stream_v, "mass kernel launch", &qp.kind,
                        err, errlen);
}

extern "C" int wo_dev_mass_sums_host(WoDev* dev, WoMassLaunch const* ml, void* sums, char* err, size_t errlen) {
    const size_t bytes = 24u * sizeof(unsigned long long);  // Wo_MassSums
    return host_round_trip(
        dev, bytes, {{nullptr, 0, bytes}}, "hipMemset(sums)",
        [&](char* io) { return wo_dev_mass_sums(dev, ml, io, dev->stream, err, errlen); }, {{sums, 0, bytes}},
        "mass query", err, errlen);
}

// ---- point classification: no node table, no KLayout, and not a ray launch ----

extern "C" int wo_dev_classify_points(WoDev* dev, void const* d_points, void* d_out, size_t n, void* stream_v,
                                      char* err, size_t errlen) {
    if (n == 0) return 0;
    if (!dev->d_prog) {
        snprintf(err, errlen, "no scene on the device");
        return -1;
    }
    if (((uintptr_t)d_points & 15u) || ((uintptr_t)d_out & 3u)) {
        snprintf(err, errlen, "the point buffer must be 16-byte aligned (the result buffer 4-byte)");
        return -1;
    }
    if (use_device(dev, err, errlen)) return -1;
    // the program in LDS where it fits (the kernel keeps no per-wave scratch)
    const size_t prog_bytes = (size_t)dev->n_recs * sizeof(WoRec);
    const bool in_lds = prog_bytes <= kLdsBudget;
    const void* kernel =
        in_lds ? (const void*)classify_points_kernel<true> : (const void*)classify_points_kernel<false>;
    const float4* pts = (const float4*)d_points;
    uint32_t* out = (uint32_t*)d_out;
    uint64_t n64 = n;
    void* args[] = {&dev->d_prog, &dev->n_recs, &pts, &out, &n64};
    return query_launch(dev, kernel, in_lds ? prog_bytes : 0, n, args, (hipStream_t)stream_v, "point kernel launch",
                        nullptr, err, errlen);
}

extern "C" int wo_dev_classify_points_host(WoDev* dev, void const* points, void* out, size_t n, char* err,
                                           size_t errlen) {
    if (n == 0) return 0;
    // the points (one row each), then one word per point
    const size_t pbytes = n * sizeof(float4), obytes = n * sizeof(uint32_t);
    return host_round_trip(
        dev, pbytes + obytes, {{const_cast<void*>(points), 0, pbytes}}, "hipMemcpy(points)",
        [&](char* io) { return wo_dev_classify_points(dev, io, io + pbytes, n, dev->stream, err, errlen); },
        {{out, pbytes, obytes}}, "point query", err, errlen);
}

// ---- surface mesh of the solid: seven launches in order on one stream; not a ray launch ----

// WOLOLO_MESH_PASSES = 1 .. 5 (measurement, tools/mesh_bench.py): stop after the corner pass, the
// count, the scan, the edges, the vertices; the mesh is then incomplete.
static int mesh_passes() {
    const char* v = getenv("WOLOLO_MESH_PASSES");
    const int n = v && *v ? atoi(v) : 5;
    return n >= 1 && n <= 5 ? n : 5;
}

extern "C" int wo_dev_mesh(WoDev* dev, WoMeshLaunch const* ml_in, void* d_vertices, void* d_quads, void* d_quad_ids,
                           void* d_counts, void* d_scratch, void* stream_v, char* err, size_t errlen) {
    if (scene_check(dev, err, errlen)) return -1;
    if (use_device(dev, err, errlen)) return -1;
    WoMeshLaunch ml = *ml_in;
    const WoMeshLayout lay = wo_mesh_layout(ml.n);
    char* scratch = reinterpret_cast<char*>(d_scratch);
    MeshBufs mb;
    mb.bits = reinterpret_cast<uint64_t*>(scratch + lay.bits_off);
    mb.masks = reinterpret_cast<uint64_t*>(scratch + lay.masks_off);
    mb.wcnt = reinterpret_cast<uint2*>(scratch + lay.wcnt_off);
    mb.chunks = reinterpret_cast<uint2*>(scratch + lay.chunks_off);
    mb.cross = reinterpret_cast<float*>(scratch + lay.cross_off);
    mb.vertices = (float4*)d_vertices;
    mb.quads = (uint4*)d_quads;
    mb.ids = (uint4*)d_quad_ids;
    mb.counts = (uint32_t*)d_counts;
    mb.nodes = dev->d_nodes;
    mb.n_mats = dev->n_mats;
    // (plain copies: a launch takes the address of each argument)
    uint64_t *bits = mb.bits, *masks = mb.masks;
    uint2 *wcnt = mb.wcnt, *chunks = mb.chunks;
    uint32_t* counts = mb.counts;
    if (!mb.vertices) ml.max_vertices = 0u;
    if (!mb.quads) ml.max_quads = 0u;
    // the program in LDS where it fits (the walking kernels keep no per-wave scratch), as for the points
    const size_t prog_bytes = (size_t)dev->n_recs * sizeof(WoRec);
    const bool in_lds = prog_bytes <= kLdsBudget;
    const size_t walk_lds = in_lds ? prog_bytes : 0;
    hipStream_t stream = (hipStream_t)stream_v;
    const size_t word_lanes = (size_t)lay.words * 64u, chunk_lanes = (size_t)lay.chunks * kBlock;
    const int passes = mesh_passes();
    {
        void* args[] = {&dev->d_prog, &dev->n_recs, &ml, &bits};
        if (query_launch(dev, in_lds ? (const void*)mesh_corners_kernel<true> : (const void*)mesh_corners_kernel<false>,
                         walk_lds, word_lanes, args, stream, "mesh corner kernel launch", nullptr, err, errlen))
            return -1;
    }
    if (passes < 2) return 0;
    {
        void* args[] = {&ml, &bits, &masks, &wcnt};
        if (query_launch(dev, (const void*)mesh_count_kernel, 0, word_lanes, args, stream, "mesh count kernel launch",
                         nullptr, err, errlen))
            return -1;
    }
    if (passes < 3) return 0;
    {
        void* sums[] = {&ml, &wcnt, &chunks};
        void* scan[] = {&ml, &chunks, &counts};
        void* words[] = {&ml, &wcnt, &chunks};
        if (query_launch(dev, (const void*)mesh_chunk_sums_kernel, 0, chunk_lanes, sums, stream,
                         "mesh scan kernel launch", nullptr, err, errlen) ||
            query_launch(dev, (const void*)mesh_scan_chunks_kernel, 0, kBlock, scan, stream, "mesh scan kernel launch",
                         nullptr, err, errlen) ||
            query_launch(dev, (const void*)mesh_scan_words_kernel, 0, chunk_lanes, words, stream,
                         "mesh scan kernel launch", nullptr, err, errlen))
            return -1;
    }
    if (passes < 4) return 0;
    {
        // the quads' number is the device's alone: a resident grid, whose loops end at the count
        void* args[] = {&dev->d_prog, &dev->n_recs, &ml, &mb};
        if (query_launch(dev, in_lds ? (const void*)mesh_edges_kernel<true> : (const void*)mesh_edges_kernel<false>,
                         walk_lds, (size_t)lay.corners * 3u, args, stream, "mesh edge kernel launch", nullptr, err, errlen))
            return -1;
    }
    if (passes < 5 || ml.max_vertices == 0u) return 0;
    void* args[] = {&ml, &mb};
    return query_launch(dev, (const void*)mesh_vertices_kernel, 0, word_lanes, args, stream, "mesh vertex kernel launch",
                        nullptr, err, errlen);
}

extern "C" int wo_dev_mesh_host(WoDev* dev, WoMeshLaunch const* ml, void* vertices, void* quads, void* quad_ids,
                                void* counts, char* err, size_t errlen) {
    // the counts (one row), the scratch, then the vertex, quad and id rows
    const size_t row = 16u, scratch = (wo_mesh_layout(ml->n).bytes + 15u) & ~(size_t)15u;
    const size_t vbytes = vertices ? (size_t)ml->max_vertices * row : 0u, qbytes = quads ? (size_t)ml->max_quads * row : 0u;
    const size_t ibytes = quads && quad_ids ? qbytes : 0u;
    const size_t voff = row + scratch, qoff = voff + vbytes, ioff = qoff + qbytes;
    return host_round_trip(
        dev, ioff + ibytes, {}, "",
        [&](char* io) {
            return wo_dev_mesh(dev, ml, vbytes ? io + voff : nullptr, qbytes ? io + qoff : nullptr,
                               ibytes ? io + ioff : nullptr, io, io + row, dev->stream, err, errlen);
        },
        {{counts, 0, row}, {vertices, voff, vbytes}, {quads, qoff, qbytes}, {quad_ids, ioff, ibytes}}, "mesh query", err,
        errlen);
}
