// mesh_kernels.h -- the surface mesh of the solid (renderer_ext.h "surface mesh of the solid":
// naive surface nets on a uniform grid) for gfx950, device code only.  query_launch.hip
// instantiates and launches the kernels; it includes wo_dev.h first (WoMeshLaunch, a kernel
// argument, and WO_MESH_CHUNK_WORDS are declared there, beside the scratch layout).
//
// Seven launches on one stream, every one a grid-stride loop over work numbered without
// regard to the grid, so no row depends on launch geometry:
//   corners   one lane per corner, 64 corners (a "word") per wave trip: the coordinate is made
//             in the kernel, the program is walked once by the wave (as classify_points_kernel
//             walks it), and the wave's __ballot is the word's inside bits (outer layer forced 0);
//   count     one lane per corner: the corner's cell is active and its +x, +y, +z edges are
//             taken, by the bit array; four ballots and two counts per word;
//   scan      three launches: per chunk of 1024 words the sums, one workgroup's exclusive scan
//             of the chunks (it also writes Wo_MeshCounts), per chunk the words' exclusive
//             prefixes.  A cell's vertex index is prefix + popcount(active mask below the lane),
//             a quad's the same over the three edge masks in (lane, axis) order;
//   edges     one lane per quad, full waves from the compacted numbering: the lane finds its
//             edge by bisecting the prefixes, bisects the edge (`iters` walks), makes the two
//             attributing walks (one walk over both points), stores the crossing by corner and
//             axis, and writes the quad's four vertex indices and ids; caps are counted;
//   vertices  one lane per corner of a word with an active cell: the up to 12 crossings in
//             the fixed order, the division, the row.
#pragma once
#include "wo_tracers.h"

namespace {

constexpr uint32_t kMeshNone = 0xFFFFFFFFu;
constexpr uint32_t kMeshQuadPositive = 4u, kMeshQuadCap = 8u;  // WO_MESH_QUAD_* (renderer_ext.h)
constexpr uint32_t kWavesPerBlock = kBlock / 64u;

// The kernels' view of the buffers: the scratch sections (wo_dev.h wo_mesh_layout) and the outputs.
struct MeshBufs {
    uint64_t* __restrict__ bits;    // [words] inside bits
    uint64_t* __restrict__ masks;   // [words][4] active cell, taken x, y, z edge
    uint2* __restrict__ wcnt;       // [words] (vertices, quads): counts, then exclusive prefixes
    uint2* __restrict__ chunks;     // [chunks] likewise
    float* __restrict__ cross;      // [corners][3] the crossing of a taken edge
    float4* __restrict__ vertices;  // Wo_MeshVertex rows, or nullptr
    uint4* __restrict__ quads;      // Wo_MeshQuad rows, or nullptr
    uint4* __restrict__ ids;        // Wo_MeshQuadIds rows, or nullptr
    uint32_t* __restrict__ counts;  // Wo_MeshCounts
    const uint32_t* __restrict__ nodes;  // per program record: its source node handle
    uint32_t n_mats;
};

// The grid's corner counts per axis, its corners and words.
struct MeshDims {
    uint32_t N0, N1, N01, corners, words;
    __device__ __forceinline__ explicit MeshDims(const WoMeshLaunch& ml) {
        N0 = ml.n[0] + 1u;
        N1 = ml.n[1] + 1u;
        N01 = N0 * N1;
        corners = N01 * (ml.n[2] + 1u);  // at most 1025^3 < 2^31
        words = (corners + 63u) >> 6;
    }
    __device__ __forceinline__ void ijk(uint32_t c, uint32_t& i, uint32_t& j, uint32_t& k) const {
        k = c / N01;
        const uint32_t r = c - k * N01;
        j = r / N0;
        i = r - j * N0;
    }
};

__device__ __forceinline__ uint64_t mesh_below(uint32_t lane) { return (1ull << lane) - 1ull; }  // lane < 64
__device__ __forceinline__ uint32_t mesh_bit(const uint64_t* __restrict__ words, uint32_t c) {
    return (uint32_t)(words[c >> 6] >> (c & 63u)) & 1u;
}
// c_a(i) = lo[a] + (float)i * h[a]: a product, then a sum
__device__ __forceinline__ float mesh_coord(const WoMeshLaunch& ml, int a, uint32_t i) {
    const float step = (float)i * ml.h[a];
    return ml.lo[a] + step;
}

// One leaf's own test of point classification: v <= f[3].
__device__ __forceinline__ bool mesh_leaf_test(const WoRec& L, uint32_t op, float px, float py, float pz) {
    float v;
    if (op == WO_LEAF_SPHERE) {
        const float gx = px - L.f[0], gy = py - L.f[1], gz = pz - L.f[2];
        v = (gx * gx + gy * gy) + gz * gz;
    } else {
        v = (L.f[0] * px + L.f[1] * py) + L.f[2] * pz;
    }
    return v <= L.f[3];
}

// Point classification of one point per lane, the program walked once by the wave (every
// lane of the wave calls it together): classify_points_kernel's walk, BOUND records stepped over.
__device__ __forceinline__ bool mesh_inside(const ProgPtr& prog, uint32_t nrec, float px, float py, float pz) {
    constexpr uint32_t kTruth = InterpTracer<false>::kTruth;
    uint32_t st = 0, pc = 0;
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
                inside = inside & mesh_leaf_test(L, uni(L.op), px, py, pz);
            }
            st = (st << 1) | (inside ? 1u : 0u);
            pc += 1u + count;
        } else {
            const uint32_t tt = (kTruth >> (4u * op)) & 15u;
            st = ((st >> 2) << 1) | ((tt >> (st & 3u)) & 1u);
            ++pc;
        }
    }
    return (st & 1u) != 0u;
}

// The two attributing walks as one: the classification of points a and b, and the first leaf
// record, in program order, whose own test differs between them (kMeshNone: none does).
__device__ __forceinline__ void mesh_attribute(const ProgPtr& prog, uint32_t nrec, float ax, float ay, float az, float bx,
                                               float by, float bz, bool& in_a, bool& in_b, uint32_t& leaf) {
    constexpr uint32_t kTruth = InterpTracer<false>::kTruth;
    uint32_t sa = 0, sb = 0, pc = 0;
    leaf = kMeshNone;
    while (pc < nrec) {
        const WoRec rec = prog[pc];
        const uint32_t op = uni(rec.op);
        if (op == WO_OP_BOUND) {
            ++pc;
        } else if (op == WO_OP_PRIM) {
            const uint32_t count = uni(rec.u0);
            bool ia = true, ib = true;
            for (uint32_t m = 0; m < count; ++m) {
                const WoRec L = prog[pc + 1u + m];
                const uint32_t lop = uni(L.op);
                const bool ta = mesh_leaf_test(L, lop, ax, ay, az), tb = mesh_leaf_test(L, lop, bx, by, bz);
                if ((ta != tb) & (leaf == kMeshNone)) leaf = pc + 1u + m;
                ia = ia & ta;
                ib = ib & tb;
            }
            sa = (sa << 1) | (ia ? 1u : 0u);
            sb = (sb << 1) | (ib ? 1u : 0u);
            pc += 1u + count;
        } else {
            const uint32_t tt = (kTruth >> (4u * op)) & 15u;
            sa = ((sa >> 2) << 1) | ((tt >> (sa & 3u)) & 1u);
            sb = ((sb >> 2) << 1) | ((tt >> (sb & 3u)) & 1u);
            ++pc;
        }
    }
    in_a = (sa & 1u) != 0u;
    in_b = (sb & 1u) != 0u;
}

// ---- corners ----
template <bool kProgInLds>
__global__ __launch_bounds__(kBlock) void mesh_corners_kernel(const WoRec* __restrict__ gprog, uint32_t nrec,
                                                              WoMeshLaunch ml, uint64_t* __restrict__ bits) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    ProgPtr prog;
    stage_program<kProgInLds>(prog, smem, gprog, nrec, threadIdx.x);
    const MeshDims d(ml);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * kWavesPerBlock;
    // (every lane of a wave runs the same trips: the word is the wave's, the walk wave-uniform)
    for (uint32_t w = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); w < d.words; w += stride) {
        const uint32_t c = w * 64u + lane;
        const bool valid = c < d.corners;
        uint32_t i, j, k;
        d.ijk(valid ? c : 0u, i, j, k);
        const bool interior = (i > 0u) & (i < ml.n[0]) & (j > 0u) & (j < ml.n[1]) & (k > 0u) & (k < ml.n[2]);
        const bool in = mesh_inside(prog, nrec, mesh_coord(ml, 0, i), mesh_coord(ml, 1, j), mesh_coord(ml, 2, k));
        const uint64_t word = __ballot(in & valid & interior);
        if (lane == 0u) bits[w] = word;
    }
}

// ---- count ----
__global__ __launch_bounds__(kBlock) void mesh_count_kernel(WoMeshLaunch ml, const uint64_t* __restrict__ bits,
                                                            uint64_t* __restrict__ masks, uint2* __restrict__ wcnt) {
    const MeshDims d(ml);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * kWavesPerBlock;
    for (uint32_t w = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); w < d.words; w += stride) {
        const uint32_t c = w * 64u + lane;
        bool x = false, y = false, z = false, active = false;
        if (c < d.corners) {
            uint32_t i, j, k;
            d.ijk(c, i, j, k);
            const bool hx = i < ml.n[0], hy = j < ml.n[1], hz = k < ml.n[2];  // the corner has a +x, +y, +z edge
            const uint32_t b0 = mesh_bit(bits, c);
            const uint32_t bx = hx ? mesh_bit(bits, c + 1u) : b0;
            const uint32_t by = hy ? mesh_bit(bits, c + d.N0) : b0;
            const uint32_t bz = hz ? mesh_bit(bits, c + d.N01) : b0;
            x = bx != b0;
            y = by != b0;
            z = bz != b0;
            if (hx & hy & hz) {  // the corner is a cell's: any of its 12 edges is taken iff its 8 bits are not all equal
                const uint32_t sum = b0 + bx + by + bz + mesh_bit(bits, c + 1u + d.N0) + mesh_bit(bits, c + 1u + d.N01) +
                                     mesh_bit(bits, c + d.N0 + d.N01) + mesh_bit(bits, c + 1u + d.N0 + d.N01);
                active = (sum != 0u) & (sum != 8u);
            }
        }
        const uint64_t ma = __ballot(active), mx = __ballot(x), my = __ballot(y), mz = __ballot(z);
        if (lane == 0u) {
            masks[4u * (size_t)w] = ma;
            masks[4u * (size_t)w + 1u] = mx;
            masks[4u * (size_t)w + 2u] = my;
            masks[4u * (size_t)w + 3u] = mz;
            wcnt[w] = make_uint2((uint32_t)__popcll(ma), (uint32_t)(__popcll(mx) + __popcll(my) + __popcll(mz)));
        }
    }
}

// ---- scan ----
// The workgroup's inclusive scan of one (vertices, quads) pair per thread; `total` is the
// workgroup's sum.  Called by every thread; `sh` holds one pair per wave.
__device__ __forceinline__ uint2 mesh_block_scan(uint2 v, uint2* sh, uint2& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t s = 1u; s < 64u; s <<= 1) {
        const uint32_t ox = __shfl_up(v.x, s, 64), oy = __shfl_up(v.y, s, 64);
        if (lane >= s) {
            v.x += ox;
            v.y += oy;
        }
    }
    __syncthreads();  // the previous call's readers are done with sh
    if (lane == 63u) sh[wave] = v;
    __syncthreads();
    total = make_uint2(0u, 0u);
#pragma unroll
    for (uint32_t q = 0; q < kWavesPerBlock; ++q) {
        const uint2 t = sh[q];
        if (q < wave) {
            v.x += t.x;
            v.y += t.y;
        }
        total.x += t.x;
        total.y += t.y;
    }
    return v;
}

// Each thread's four consecutive words of chunk `ch` (zero past the last word).
__device__ __forceinline__ void mesh_chunk_words(const uint2* __restrict__ wcnt, uint32_t words, uint32_t ch, uint2 v[4]) {
    const uint32_t w0 = ch * WO_MESH_CHUNK_WORDS + threadIdx.x * 4u;
#pragma unroll
    for (uint32_t t = 0; t < 4u; ++t) v[t] = w0 + t < words ? wcnt[w0 + t] : make_uint2(0u, 0u);
}
static_assert(WO_MESH_CHUNK_WORDS == 4u * kBlock, "a thread scans four words of a chunk");

__global__ __launch_bounds__(kBlock) void mesh_chunk_sums_kernel(WoMeshLaunch ml, const uint2* __restrict__ wcnt,
                                                                 uint2* __restrict__ chunks) {
    __shared__ uint2 sh[kWavesPerBlock];
    const MeshDims d(ml);
    const uint32_t nchunks = (d.words + WO_MESH_CHUNK_WORDS - 1u) / WO_MESH_CHUNK_WORDS;
    for (uint32_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        uint2 v[4];
        mesh_chunk_words(wcnt, d.words, ch, v);
        uint2 total;
        (void)mesh_block_scan(make_uint2(v[0].x + v[1].x + v[2].x + v[3].x, v[0].y + v[1].y + v[2].y + v[3].y), sh, total);
        if (threadIdx.x == 0u) chunks[ch] = total;
    }
}

// One workgroup: the chunks' exclusive prefixes in place, then the counts (cap_quads starts at 0:
// the edge pass adds to it).
__global__ __launch_bounds__(kBlock) void mesh_scan_chunks_kernel(WoMeshLaunch ml, uint2* __restrict__ chunks,
                                                                  uint32_t* __restrict__ counts) {
    __shared__ uint2 sh[kWavesPerBlock];
    if (blockIdx.x != 0u) return;
    const MeshDims d(ml);
    const uint32_t nchunks = (d.words + WO_MESH_CHUNK_WORDS - 1u) / WO_MESH_CHUNK_WORDS;
    uint2 carry = make_uint2(0u, 0u);
    for (uint32_t base = 0; base < nchunks; base += kBlock) {
        const uint32_t idx = base + threadIdx.x;
        const uint2 own = idx < nchunks ? chunks[idx] : make_uint2(0u, 0u);
        uint2 total;
        const uint2 incl = mesh_block_scan(own, sh, total);
        if (idx < nchunks) chunks[idx] = make_uint2(carry.x + incl.x - own.x, carry.y + incl.y - own.y);
        carry.x += total.x;
        carry.y += total.y;
    }
    if (threadIdx.x == 0u) {
        counts[0] = carry.x;
        counts[1] = carry.y;
        counts[2] = 0u;
        counts[3] = ((carry.x > ml.max_vertices) | (carry.y > ml.max_quads)) ? 1u : 0u;  // WO_MESH_TRUNCATED
    }
}

__global__ __launch_bounds__(kBlock) void mesh_scan_words_kernel(WoMeshLaunch ml, uint2* __restrict__ wcnt,
                                                                 const uint2* __restrict__ chunks) {
    __shared__ uint2 sh[kWavesPerBlock];
    const MeshDims d(ml);
    const uint32_t nchunks = (d.words + WO_MESH_CHUNK_WORDS - 1u) / WO_MESH_CHUNK_WORDS;
    for (uint32_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        uint2 v[4];
        mesh_chunk_words(wcnt, d.words, ch, v);
        const uint2 own = make_uint2(v[0].x + v[1].x + v[2].x + v[3].x, v[0].y + v[1].y + v[2].y + v[3].y);
        uint2 total;
        const uint2 incl = mesh_block_scan(own, sh, total);
        const uint2 off = chunks[ch];
        uint2 run = make_uint2(off.x + incl.x - own.x, off.y + incl.y - own.y);
        const uint32_t w0 = ch * WO_MESH_CHUNK_WORDS + threadIdx.x * 4u;
#pragma unroll
        for (uint32_t t = 0; t < 4u; ++t) {
            if (w0 + t < d.words) wcnt[w0 + t] = run;
            run.x += v[t].x;
            run.y += v[t].y;
        }
    }
}

// ---- edges ----
// The vertex index of the cell whose low corner is corner `cc`.
__device__ __forceinline__ uint32_t mesh_vertex_index(const MeshBufs& mb, uint32_t cc) {
    return mb.wcnt[cc >> 6].x + (uint32_t)__popcll(mb.masks[4u * (size_t)(cc >> 6)] & mesh_below(cc & 63u));
}

template <bool kProgInLds>
__global__ __launch_bounds__(kBlock) void mesh_edges_kernel(const WoRec* __restrict__ gprog, uint32_t nrec,
                                                            WoMeshLaunch ml, MeshBufs mb) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    ProgPtr prog;
    stage_program<kProgInLds>(prog, smem, gprog, nrec, threadIdx.x);
    const MeshDims d(ml);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nquads = mb.counts[1];  // the scan's, complete before this launch
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    // (every lane of a wave runs the same trips: the bound is the wave's, the walks wave-uniform)
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u); base < nquads; base += stride) {
        const bool live = base + lane < nquads;
        const uint32_t q = live ? (uint32_t)(base + lane) : nquads - 1u;  // an idle lane repeats the last quad, writes nothing
        // the quad's word: the last one whose prefix is <= q (it holds quads: the next prefix is larger)
        uint32_t wlo = 0u, whi = d.words - 1u;
        while (wlo < whi) {
            const uint32_t mid = wlo + ((whi - wlo + 1u) >> 1);
            if (mb.wcnt[mid].y <= q)
                wlo = mid;
            else
                whi = mid - 1u;
        }
        const uint32_t w = wlo;
        const uint64_t mx = mb.masks[4u * (size_t)w + 1u], my = mb.masks[4u * (size_t)w + 2u], mz = mb.masks[4u * (size_t)w + 3u];
        uint32_t r = q - mb.wcnt[w].y;  // the quad's rank in the word's (lane, axis) order
        // its lane: the last one with at most r of the word's edges below it
        uint32_t llo = 0u, lhi = 63u;
        while (llo < lhi) {
            const uint32_t mid = (llo + lhi + 1u) >> 1;
            const uint64_t below = mesh_below(mid);
            if ((uint32_t)(__popcll(mx & below) + __popcll(my & below) + __popcll(mz & below)) <= r)
                llo = mid;
            else
                lhi = mid - 1u;
        }
        const uint32_t l = llo;
        {
            const uint64_t below = mesh_below(l);
            r -= (uint32_t)(__popcll(mx & below) + __popcll(my & below) + __popcll(mz & below));
        }
        const uint32_t ex = (uint32_t)(mx >> l) & 1u, ey = (uint32_t)(my >> l) & 1u;
        const uint32_t a = r < ex ? 0u : (r < ex + ey ? 1u : 2u);  // the r-th of the lane's taken edges
        const uint32_t c = w * 64u + l;
        uint32_t i, j, k;
        d.ijk(c, i, j, k);
        const float px = mesh_coord(ml, 0, i), py = mesh_coord(ml, 1, j), pz = mesh_coord(ml, 2, k);
        const bool sa = mesh_bit(mb.bits, c) != 0u;
        float ta = a == 0u ? px : (a == 1u ? py : pz);
        float tb = a == 0u ? mesh_coord(ml, 0, i + 1u) : (a == 1u ? mesh_coord(ml, 1, j + 1u) : mesh_coord(ml, 2, k + 1u));
        for (uint32_t it = 0; it < ml.iters; ++it) {
            const float sum = ta + tb;
            const float tm = 0.5f * sum;
            const bool sm = mesh_inside(prog, nrec, a == 0u ? tm : px, a == 1u ? tm : py, a == 2u ? tm : pz);
            if (sm == sa)
                ta = tm;
            else
                tb = tm;
        }
        const float xsum = ta + tb;
        if (live) mb.cross[(size_t)c * 3u + a] = 0.5f * xsum;
        bool in_a, in_b;
        uint32_t leaf;
        mesh_attribute(prog, nrec, a == 0u ? ta : px, a == 1u ? ta : py, a == 2u ? ta : pz, a == 0u ? tb : px,
                       a == 1u ? tb : py, a == 2u ? tb : pz, in_a, in_b, leaf);
        const bool cap = (in_a == in_b) | (leaf == kMeshNone);
        const uint64_t caps = __ballot(live & cap);
        if (lane == 0u && caps != 0ull) (void)atomicAdd(&mb.counts[2], (uint32_t)__popcll(caps));
        if (!live || q >= ml.max_quads) continue;
        // the four cells round the edge, at (u, v) offsets (-1,-1), (0,-1), (0,0), (-1,0) of the lower corner's
        // cell coordinates; u = (a+1)%3, v = (a+2)%3.  All exist (a taken edge has an interior end); a corner
        // on the low faces would wrap, so such a quad -- there is none -- is not written.
        const uint32_t iu = a == 0u ? j : (a == 1u ? k : i), iv = a == 0u ? k : (a == 1u ? i : j);
        if (iu == 0u || iv == 0u) continue;
        const uint32_t su = a == 0u ? d.N0 : (a == 1u ? d.N01 : 1u), sv = a == 0u ? d.N01 : (a == 1u ? 1u : d.N0);
        const uint32_t v0 = mesh_vertex_index(mb, c - su - sv), v1 = mesh_vertex_index(mb, c - sv);
        const uint32_t v2 = mesh_vertex_index(mb, c), v3 = mesh_vertex_index(mb, c - su);
        mb.quads[q] = sa ? make_uint4(v0, v1, v2, v3) : make_uint4(v3, v2, v1, v0);
        if (mb.ids) {
            const uint32_t flags = a | (sa ? kMeshQuadPositive : 0u) | (cap ? kMeshQuadCap : 0u);
            uint4 row = make_uint4(kMeshNone, kMeshNone, kMeshNone, flags);
            if (!cap) {
                const WoRec L = prog[leaf];
                row = make_uint4(leaf, mb.nodes[leaf], L.u0 < mb.n_mats ? L.u0 : 0u, flags);
            }
            mb.ids[q] = row;
        }
    }
}

// ---- vertices ----
__global__ __launch_bounds__(kBlock) void mesh_vertices_kernel(WoMeshLaunch ml, MeshBufs mb) {
    const MeshDims d(ml);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t stride = gridDim.x * kWavesPerBlock;
    for (uint32_t w = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); w < d.words; w += stride) {
        const uint64_t active = mb.masks[4u * (size_t)w];
        if (((active >> lane) & 1ull) == 0ull) continue;
        const uint32_t vi = mb.wcnt[w].x + (uint32_t)__popcll(active & mesh_below(lane));
        if (vi >= ml.max_vertices) continue;
        const uint32_t c = w * 64u + lane;
        uint32_t idx[3];
        d.ijk(c, idx[0], idx[1], idx[2]);
        const uint32_t step[3] = {1u, d.N0, d.N01};
        float sum[3] = {0.0f, 0.0f, 0.0f};
        uint32_t count = 0u;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int u = (a + 1) % 3, v = (a + 2) % 3;
#pragma unroll
            for (uint32_t dv = 0; dv < 2u; ++dv) {
#pragma unroll
                for (uint32_t du = 0; du < 2u; ++du) {
                    const uint32_t ce = c + du * step[u] + dv * step[v];
                    const uint64_t taken = mb.masks[4u * (size_t)(ce >> 6) + 1u + (uint32_t)a];
                    if (((taken >> (ce & 63u)) & 1ull) != 0ull) {
                        sum[a] += mb.cross[(size_t)ce * 3u + (uint32_t)a];
                        sum[u] += mesh_coord(ml, u, idx[u] + du);
                        sum[v] += mesh_coord(ml, v, idx[v] + dv);
                        ++count;
                    }
                }
            }
        }
        const float n = (float)count;  // >= 1: the cell is active
        const uint32_t cell = (idx[2] * ml.n[1] + idx[1]) * ml.n[0] + idx[0];
        mb.vertices[vi] = make_float4(__fdiv_rn(sum[0], n), __fdiv_rn(sum[1], n), __fdiv_rn(sum[2], n), __uint_as_float(cell));
    }
}

}  // namespace
