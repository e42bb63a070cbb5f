// wo_dev_impl.h -- what the library's two HIP units share on the host side: the device object
// behind wo_dev.h's handle, the kernel kinds, and the few helpers both the frame path
// (trace_kernels.hip) and the query path (query_launch.hip) call.  Included by those two
// units only, after wo_tracers.h.  The helpers are defined here (static inline), not only
// declared: interp_plan and lane_bvh fill kernel-argument structs (KLayout, LaneBvh) that
// live in wo_tracers.h's unnamed namespace, so they cannot link across units.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "wo_tracers.h"
#include "wo_dev.h"

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

static inline void set_err(char* err, size_t len, const char* what, hipError_t e) {
    if (err && len) snprintf(err, len, "%s: %s", what, hipGetErrorString(e));
}

template <class T>
static inline int ensure_buffer(T** p, size_t* cap, size_t bytes, char* err, size_t errlen) {
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
static inline LaneBvh lane_bvh(const WoDev* dev) {
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

constexpr size_t kLdsBudget = 64u * 1024u;

// the numbers are wo_renderer_lanes_info's "kind" (the lane tracer's forms, LaneTracer)
enum PathKind { kLanesBvh = 2, kLanesBvhSpheres = 3, kLanesTerms = 6, kLanesGeneral = 7, kLanesDynWideTerms = 14,
                kJit = 16, kInterpLds = 17, kInterpGlobal = 18 };

// The interpreter's per-wave LDS scratch (KLayout) for a program of n_recs records
// and n_prims primitives, and its form: the program in LDS too when both fit
// (kInterpLds), else read from global memory (kInterpGlobal).  The frame kernel
// and the query kernels share it.
static inline int interp_plan(uint32_t n_recs, uint32_t n_prims, KLayout* lay, PathKind* kind, size_t* dyn_lds,
                              char* err, size_t errlen) {
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

// Workgroups of a ray launch: one ray per lane, at most the workgroups the device
// holds at once (the grid-stride loop takes the rest).  WOLOLO_RAY_BLOCKS
// (measurement) caps the grid.
static inline uint32_t ray_grid(const WoDev* dev, size_t n, int per_cu) {
    uint64_t blocks = ((uint64_t)n + kBlock - 1u) / kBlock;
    uint64_t resident = (uint64_t)dev->cus * (uint64_t)(per_cu < 1 ? 1 : per_cu);
    const char* cap = getenv("WOLOLO_RAY_BLOCKS");
    if (cap && *cap && atoi(cap) > 0) resident = (uint64_t)atoi(cap);
    return (uint32_t)(blocks < resident ? blocks : resident);
}
