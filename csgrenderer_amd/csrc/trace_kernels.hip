// trace_kernels.hip -- the frame path of the wololo renderer on the host, for gfx950 (MI355X,
// CDNA4, wave64): the device object's lifecycle, scene, node-table and specialised-kernel
// upload, the tile plan and launch of the path kernels (path_kernels.h, instantiated here;
// wo_jit_pathtrace, the kernel specialised per scene, comes from scene_jit.c through
// jit_code.cpp and is loaded here), kernel_info, the work counters, the frame slots,
// present and the multi-device gather.  The C ABI is wo_dev.h's; the queries' half of it
// is query_launch.hip.
#include "wo_tracers.h"  // first: every define that shapes device code is made there

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
#include "path_kernels.h"
#include "wo_dev_impl.h"

#include "static_key.inc"  // WO_STATIC_SRC_SHA: the library kernels' source identity

// big tiles per resident workgroup of a rank's share (plan_tiles), every kernel;
// a generated source may name its own (`// wo_share_tiles N`, scene_jit.c)
constexpr uint32_t kShareTiles = 3u;

// Zero device memory and wait for it: hipMemset may still be running on the null
// stream when a kernel on one of the non-blocking streams starts, and a late
// memset would wipe what that kernel counted.  (One-time set-ups only.)
static hipError_t zero_now(void* p, size_t bytes) {
    hipError_t e = hipMemset(p, 0, bytes);
    return e == hipSuccess ? hipDeviceSynchronize() : e;
}

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

extern "C" int wo_dev_launch(WoDev* dev, WoFrame const* frame_in, void* d_out, void* stream_v,
                             unsigned long long* d_segments, char* err, size_t errlen) {
    return wo_dev_launch_ex(dev, frame_in, d_out, stream_v, d_segments, nullptr, 0u, err, errlen);
}

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
