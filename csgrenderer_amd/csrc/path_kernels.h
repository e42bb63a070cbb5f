// path_kernels.h -- the library's frame kernels for gfx950, device code only (the tracers are
// wo_tracers.h's).  Replaces the reference's fragment stage (src/wololo/renderer/
// ubershader1.frag:19-163, one invocation per pixel, launched by draw_frame_with_renderer,
// renderer.c:2085-2219).
//   ubershader_kernel       the reference shader restated bit-for-bit in IEEE fp32
//                           (sin hoisted to the host).  HBM-store bound, 16 B/pixel.
//   pathtrace_kernel        CSG path tracer, INTERPRETER form (InterpTracer).
//   pathtrace_lanes_kernel  the same over the lane walk's forms (LaneTracer).
//   wo_jit_pathtrace        the same path tracer SPECIALISED per scene is not here: source from
//                           scene_jit.c, compiled and cached by jit_code.cpp.
//   assemble_kernel         un-interleaves row-cyclic rank tiles after the gather.
//   srgb8_kernel, seg_collect_kernel, work_collect_kernel, fastmath_check_kernel.
// All forms agree bit-for-bit with oracle/oracle.c.
#pragma once
#include "wo_tracers.h"

namespace {

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
// Dynamic LDS: the BVH walk's lane stacks ([depth][kBlock] u32 or u16) and top nodes (WO_LANE_SETUP).
template <int kMode, bool kCount>
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
    WO_LANE_SETUP(tr, prog, ordpc, bvh, smem);  // (pathtrace_block's first barrier orders the copy of the top nodes)
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

    InterpTracer<kCount> tr;
    interp_setup<kProgInLds>(tr, smem, gprog, nrec, lay, tid, lane, wave);
    pathtrace_block(tr, mats, fr, local_rows, out, seg_slots, tg);
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
