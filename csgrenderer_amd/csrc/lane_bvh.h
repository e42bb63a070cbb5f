/*
 * lane_bvh.h -- what the lane tracer's kernels (wo_tracers.h) and the host
 * builder of its ordered BVH (lane_bvh_build.cpp) share: the descriptor of a
 * built BVH, the encodings of its packed blob, and the size of the walk's LDS.
 * The blob's sections and their order: DESIGN.md §3.6f.
 */
#ifndef WOLOLO_LANE_BVH_H
#define WOLOLO_LANE_BVH_H

#include <stddef.h>
#include <stdint.h>

#include "wololo/wo_scene.h"

/* A built lane BVH: counts, flags (0 / 1) and the u32 offsets of the blob's
 * later sections.  No lane form: union_only, terms and general are all 0. */
typedef struct WoLaneBvhDesc {
    uint32_t nprims;
    uint32_t nodes, always;
    uint32_t root;         /* 0, a leaf ref (one leaf), or kNoRef (no tree) */
    uint32_t depth;        /* entries of a lane's stack (binary: internal levels, <= kLaneDepthMax) */
    uint32_t top;          /* nodes [0, top) staged in LDS per workgroup */
    uint32_t terms;        /* term mode (kinds 6 / 14): the leaves and the always list hold terms */
    uint32_t union_only;   /* every binop is a UNION (kinds 2 / 3) */
    uint32_t spheres_only; /* and every primitive a single sphere (kind 3) */
    uint32_t stack16;      /* 16-bit stack entries (the 4-wide and the general tree) */
    uint32_t wide;         /* 4-wide nodes of 7 float4 (kind 14) */
    uint32_t general;      /* a general tree (kind 7): the BVH over its primitives, gpar / gnode / gclip */
    uint32_t term_off, leaf_off, gpar_off, gnode_off, gclip_off;
    uint32_t gP, gwords, groot; /* general tree: leaves (= primitives), bit words per lane, the root's ref */
} WoLaneBvhDesc;

#ifdef __cplusplus

#include <vector>

namespace wolbvh {

constexpr uint32_t kLeafRef = 0x80000000u, kNoRef = 0xffffffffu;
// 16-bit refs (lane stacks, 4-wide nodes): node index or ordinal in bits 0-14, leaf flag in bit 15
constexpr uint32_t kNoRef16 = 0xffffu;
// term mode: literals per term; a literal is ordinal | kLitNeg (complement)
constexpr uint32_t kTermLits = 2, kLitNeg = 0x80000000u, kNoLit = 0xffffffffu;
// term records: float4 [0] = literal 0, literal 1, kinds (2 bits per literal), 0;
// [1 + 2x], [2 + 2x] = literal x's sphere members (centre, r^2)
constexpr uint32_t kTermRecF4 = 5, kTermLitSphere = 1, kTermLitSphere2 = 2;  // kind 0: generic (prim_ivl)
// The lane BVH is built with at most kLaneDepthMax internal levels on any path,
// and the per-lane LDS stack holds as many entries as the built tree has levels:
// a walk pushes at most one sibling per ancestor, so the stack never overflows.
constexpr uint32_t kLaneDepthMax = 24;
// a general tree's node record: left ref | right ref << 15 | op << 30
// (op: 0 union, 1 intersection, 2 a AND NOT b, 3 b AND NOT a)
constexpr uint32_t kGRefBits = 15u, kGRefMask = (1u << kGRefBits) - 1u;

#ifndef WO_LANES_CAM
#define WO_LANES_CAM 0  // the lane kernels' camera-wave mode (pathtrace_block kCam)
#endif
// the camera ring's LDS per workgroup (64 slots of 48 B per wave)
constexpr size_t kCamRingLds = WO_LANES_CAM ? 4u * 64u * 48u : 0u;
// dynamic LDS of the BVH walk: 8 workgroups per CU = 20 KB each, less the kernels'
// static LDS (2224 B since the pixel-row table, round 5; at 18 KB of dynamic LDS the
// total crossed 20 KB and the RTIOW cover ran at 7 workgroups per CU: 11.24 -> 11.69 ms)
constexpr size_t kLanesStaticLdsMax = 2304u;
constexpr size_t kLanesBvhLds = 20u * 1024u - kLanesStaticLdsMax;
constexpr uint32_t kLaneBlock = 256;  // lanes of a workgroup (wodev::kBlock)

inline uint32_t lane_node_f4(const WoLaneBvhDesc& d) { return d.wide ? 7u : 4u; }

// Dynamic LDS of a lane kernel's workgroup: the lane stacks ([depth][lane], 16 bytes
// aligned), the top nodes, and a general tree's bit words ([word][lane]).
inline size_t lane_bvh_lds(const WoLaneBvhDesc& d) {
    const size_t stacks = ((size_t)d.depth * kLaneBlock * (d.stack16 ? 2u : 4u) + 15u) & ~(size_t)15u;
    const size_t bits = d.general ? (size_t)d.gwords * kLaneBlock * sizeof(uint32_t) : 0u;
    return stacks + bits + (size_t)d.top * lane_node_f4(d) * 16u;
}

// The builder's result: the descriptor, the ordinal -> program pc table the lane
// tracer reads generic primitives and hit leaves through, and the packed blob
// (empty when the program has no lane form).
struct LaneBvhBuild {
    WoLaneBvhDesc desc;
    std::vector<uint32_t> ordpc;
    std::vector<char> blob;
};
// lane_bvh_build.cpp (host only): 0, or -1 with a message in err.
int lane_bvh_build(WoRec const* prog, uint32_t n_recs, uint32_t n_prims, WoMaterial const* mats, uint32_t n_mats,
                   LaneBvhBuild* out, char* err, size_t errlen);

}  // namespace wolbvh

#endif /* __cplusplus */

#endif /* WOLOLO_LANE_BVH_H */
