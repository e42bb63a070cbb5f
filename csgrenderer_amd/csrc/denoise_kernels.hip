// denoise_kernels.hip -- the edge-avoiding a-trous denoiser's kernels for gfx950 and their
// launches (renderer_ext.h wo_denoise_device states the arithmetic; denoise.c is the same
// filter in host C, and the two agree bit for bit: fp32, one rounding per operation, no
// contraction, rcp_cr for the reciprocals, whose arguments all lie in [2^-20, 2^20]).
//
// The working image is one 16-byte row per pixel: the (demodulated) rgb and, in the w word,
// the pixel's node id, so a tap costs two 16-byte loads: that row and the normal / depth row.
//   dn_prologue_kernel   frame (+ albedo, ids) -> working image in scratch
//   dn_level_kernel      one level: working image -> the other scratch image, or, at the last
//                        level, re-modulated and with the frame's alpha, -> out
// in two forms per level: DIRECT reads its 24 neighbours from global memory (any step; the
// caches carry the reuse), LDS stages the workgroup's 32 x 16 tile plus a halo of 2 * step
// pixels of both rows in LDS behind one barrier (steps 1, 2 and 4: 23, 30 and 48 KiB).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "wo_denoise.h"
#include "wo_device_common.h"

#pragma clang fp contract(off)

namespace {

using wodev::kInf;
using wodev::rcp_cr;

constexpr uint32_t kDnBlock = 256;          // 32 x 8 lanes: a wave is two 32-pixel row pieces
constexpr int kTileW = 32, kTileRows = 8;   // lanes of a workgroup across and down
constexpr int kLdsPixels = 2;               // LDS form: pixels per lane (rows ty and ty + 8): a 32 x 16 tile
constexpr uint32_t kLdsMaxStep = 4;         // the LDS form's largest step: (32 + 16)(16 + 16) x 32 B = 48 KiB
// the step up to which `auto` takes the LDS form: every step that has one (1080p, csg32 at 4 spp, a level
// alone, tools/denoise_bench.py: LDS / direct 0.055 / 0.099, 0.063 / 0.101, 0.087 / 0.103 ms at steps 1, 2, 4)
constexpr uint32_t kAutoLdsMaxStep = 4;

enum : uint32_t { DN_COLOR = 1u, DN_NORMAL = 2u, DN_DEPTH = 4u, DN_STOP = 8u, DN_LAST = 16u, DN_DEMOD = 32u };

struct DnLevel {
    const float4* src;     // working image
    const float4* guide;   // normal.xyz, depth (NULL without DN_NORMAL and DN_DEPTH)
    float4* dst;           // the next working image, or out (DN_LAST)
    const float4* albedo;  // DN_LAST with DN_DEMOD
    const float4* color;   // DN_LAST: the frame, for its alpha
    int width, height, step;
    float kc, kn, kd;
    uint32_t flags;
};

__device__ __forceinline__ float clampf(float v, float lo, float hi) {
    const float t = v > lo ? v : lo;
    return t < hi ? t : hi;
}

__device__ __forceinline__ float edge(float d2, float k) {
    const float x = 1.0f - d2 * k;
    const float m = x > 0.0f ? x : 0.0f;
    return m * m;
}

__device__ __forceinline__ float dist2(float4 a, float4 b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}

__global__ __launch_bounds__(kDnBlock) void dn_prologue_kernel(const float4* __restrict__ color,
                                                              const float4* __restrict__ albedo,
                                                              const uint4* __restrict__ ids, float4* __restrict__ work,
                                                              size_t pixels) {
    for (size_t p = (size_t)blockIdx.x * kDnBlock + threadIdx.x; p < pixels; p += (size_t)gridDim.x * kDnBlock) {
        float4 c = color[p];
        if (albedo) {
            const float4 a = albedo[p];
            c.x = c.x * rcp_cr(clampf(a.x, 0x1p-7f, 0x1p20f));
            c.y = c.y * rcp_cr(clampf(a.y, 0x1p-7f, 0x1p20f));
            c.z = c.z * rcp_cr(clampf(a.z, 0x1p-7f, 0x1p20f));
        }
        c.w = __uint_as_float(ids ? ids[p].x : 0u);
        work[p] = c;
    }
}

// The centre (x, y)'s new value from its 25 taps; fetch_c / fetch_g give the two rows of an
// in-frame pixel.  The taps run dy outer, dx inner: the sums' order is part of the result.
template <bool GUIDE, class FetchC, class FetchG>
__device__ __forceinline__ void dn_pixel(const DnLevel& a, int x, int y, FetchC fetch_c, FetchG fetch_g) {
    const float H[3] = {0.375f, 0.25f, 0.0625f};
    const float4 cp = fetch_c(x, y, 0, 0);
    float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (GUIDE) gp = fetch_g(x, y, 0, 0);
    const bool finp = gp.w < kInf;
    const float rzp = (GUIDE && (a.flags & DN_DEPTH)) ? rcp_cr(clampf(gp.w, 0x1p-20f, 0x1p20f)) : 0.0f;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float h = H[dx < 0 ? -dx : dx] * H[dy < 0 ? -dy : dy];  // exact: the H are dyadic
            if (dx == 0 && dy == 0) {
                sx += h * cp.x, sy += h * cp.y, sz += h * cp.z;
                wsum += h;
                continue;
            }
            const int qx = x + dx * a.step, qy = y + dy * a.step;
            if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height) continue;
            const float4 cq = fetch_c(qx, qy, dx, dy);
            float e = 1.0f;
            if (a.flags & DN_COLOR) e *= edge(dist2(cq, cp), a.kc);
            if (GUIDE) {
                const float4 gq = fetch_g(qx, qy, dx, dy);
                if (a.flags & DN_NORMAL) e *= edge(dist2(gq, gp), a.kn);
                if (a.flags & DN_DEPTH) {
                    const bool finq = gq.w < kInf;
                    const float rel = (gq.w - gp.w) * rzp;
                    const float ed = e * edge(rel * rel, a.kd);
                    e = (finp && finq) ? ed : (finp != finq ? 0.0f : e);
                }
            }
            if ((a.flags & DN_STOP) && __float_as_uint(cq.w) != __float_as_uint(cp.w)) e = 0.0f;
            const float w = h * e;
            if (w > 0.0f) {
                sx += w * cq.x, sy += w * cq.y, sz += w * cq.z;
                wsum += w;
            }
        }
    }
    const float rw = rcp_cr(wsum);  // 9/64 <= wsum: the centre tap
    float4 o = make_float4(sx * rw, sy * rw, sz * rw, cp.w);
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    if (a.flags & DN_LAST) {
        if (a.flags & DN_DEMOD) {
            const float4 al = a.albedo[p];
            o.x = o.x * clampf(al.x, 0x1p-7f, 0x1p20f);
            o.y = o.y * clampf(al.y, 0x1p-7f, 0x1p20f);
            o.z = o.z * clampf(al.z, 0x1p-7f, 0x1p20f);
        }
        o.w = a.color[p].w;
    }
    a.dst[p] = o;
}

template <bool GUIDE>
__global__ __launch_bounds__(kDnBlock) void dn_level_direct_kernel(const DnLevel a) {
    const int x = (int)blockIdx.x * kTileW + (int)(threadIdx.x % kTileW);
    const int y = (int)blockIdx.y * kTileRows + (int)(threadIdx.x / kTileW);
    if (x >= a.width || y >= a.height) return;
    const float4* __restrict__ src = a.src;
    const float4* __restrict__ guide = a.guide;
    const size_t W = (size_t)a.width;
    dn_pixel<GUIDE>(
        a, x, y, [=](int qx, int qy, int, int) { return src[(size_t)qy * W + (size_t)qx]; },
        [=](int qx, int qy, int, int) { return guide[(size_t)qy * W + (size_t)qx]; });
}

// The LDS form.  The tile's image is row-major float4s, (32 + 4 step) across: the 16 lanes of
// a ds_read_b128 group lie in one 32-pixel row piece at 16 distinct consecutive 16-byte slots
// (MI355X: groups {0-3, 12-15, 20-27}, ...; the bank is (address / 4) mod 64, so 16 slots fill
// the 64 banks once), whatever the tap: conflict-free for every row pitch.  The staging
// stores run over the image linearly, 8 consecutive lanes to 8 consecutive slots.
template <bool GUIDE>
__global__ __launch_bounds__(kDnBlock) void dn_level_lds_kernel(const DnLevel a) {
    extern __shared__ float4 dn_lds[];
    const int halo = 2 * a.step;
    const int lw = kTileW + 2 * halo, lh = kTileRows * kLdsPixels + 2 * halo;
    const int ox = (int)blockIdx.x * kTileW - halo, oy = (int)blockIdx.y * (kTileRows * kLdsPixels) - halo;
    float4* lc = dn_lds;
    float4* lg = dn_lds + lw * lh;
    const size_t W = (size_t)a.width;
    for (int i = (int)threadIdx.x; i < lw * lh; i += (int)kDnBlock) {
        const int ly = i / lw, lx = i - ly * lw;
        const int gx = ox + lx, gy = oy + ly;
        const bool in = gx >= 0 && gx < a.width && gy >= 0 && gy < a.height;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = c;  // outside the frame: never read as a tap
        if (in) {
            c = a.src[(size_t)gy * W + (size_t)gx];
            if (GUIDE) g = a.guide[(size_t)gy * W + (size_t)gx];
        }
        lc[i] = c;
        if (GUIDE) lg[i] = g;
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x % kTileW), ty = (int)(threadIdx.x / kTileW);
    const int x = (int)blockIdx.x * kTileW + tx;
#pragma unroll
    for (int r = 0; r < kLdsPixels; ++r) {
        const int y = (int)blockIdx.y * (kTileRows * kLdsPixels) + ty + r * kTileRows;
        if (x >= a.width || y >= a.height) continue;
        dn_pixel<GUIDE>(
            a, x, y, [=](int qx, int qy, int, int) { return lc[(qy - oy) * lw + (qx - ox)]; },
            [=](int qx, int qy, int, int) { return lg[(qy - oy) * lw + (qx - ox)]; });
    }
}

int form_of_env() {  // 0 auto, 1 direct, 2 lds
    const char* f = getenv("WOLOLO_DENOISE_FORM");
    if (f && !strcmp(f, "direct")) return 1;
    if (f && !strcmp(f, "lds")) return 2;
    return 0;
}

size_t lds_bytes(uint32_t step, bool guide) {
    const size_t lw = kTileW + 4u * step, lh = (size_t)kTileRows * kLdsPixels + 4u * step;
    return lw * lh * sizeof(float4) * (guide ? 2u : 1u);
}

void set_err(char* err, size_t len, const char* what, hipError_t e) {
    if (err && len) snprintf(err, len, "%s: %s", what, hipGetErrorString(e));
}

}  // namespace

extern "C" int wo_dev_denoise(Wo_DenoiseParams const* dp, uint32_t width, uint32_t height, void const* d_color,
                              void const* d_albedo, void const* d_normal, void const* d_ids, void* d_out,
                              void* d_scratch, void* stream_v, char* err, size_t errlen) {
    hipStream_t stream = (hipStream_t)stream_v;  // NULL = the null stream (HIP convention)
    const size_t pixels = (size_t)width * height;
    float4* work[2] = {(float4*)d_scratch, (float4*)d_scratch + pixels};  // the second only for levels > 1
    const bool demod = (dp->flags & WO_DENOISE_DEMODULATE) != 0u;
    const bool guide = dp->k_normal > 0.0f || dp->k_depth > 0.0f;
    uint32_t flags = (dp->k_color > 0.0f ? DN_COLOR : 0u) | (dp->k_normal > 0.0f ? DN_NORMAL : 0u) |
                     (dp->k_depth > 0.0f ? DN_DEPTH : 0u) | ((dp->flags & WO_DENOISE_STOP_AT_NODES) ? DN_STOP : 0u) |
                     (demod ? DN_DEMOD : 0u);
    // WOLOLO_DENOISE_ONLY_LEVEL = i (measurement, tools/denoise_bench.py): launch level i's kernel alone,
    // from the first scratch image as an earlier call left it into the second (the last level: into d_out);
    // what it writes is no denoised frame
    const char* only_s = getenv("WOLOLO_DENOISE_ONLY_LEVEL");
    const int only = only_s && *only_s ? atoi(only_s) : -1;
    const bool one = only >= 0 && (uint32_t)only < dp->levels && dp->levels > 1u;
    hipError_t e = hipSuccess;
    if (!one) {
        size_t blocks = (pixels + kDnBlock - 1u) / kDnBlock;
        if (blocks > 16384u) blocks = 16384u;
        hipLaunchKernelGGL(dn_prologue_kernel, dim3((uint32_t)blocks), dim3(kDnBlock), 0, stream, (const float4*)d_color,
                           demod ? (const float4*)d_albedo : nullptr,
                           (dp->flags & WO_DENOISE_STOP_AT_NODES) ? (const uint4*)d_ids : nullptr, work[0], pixels);
        e = hipGetLastError();
        if (e != hipSuccess) {
            set_err(err, errlen, "denoise prologue launch", e);
            return -1;
        }
    }
    const int form = form_of_env();
    for (uint32_t level = one ? (uint32_t)only : 0u; level < (one ? (uint32_t)only + 1u : dp->levels); ++level) {
        const bool last = level + 1u == dp->levels;
        DnLevel a;
        a.src = one ? work[0] : work[level & 1u];
        a.guide = guide ? (const float4*)d_normal : nullptr;
        a.dst = last ? (float4*)d_out : (one ? work[1] : work[(level + 1u) & 1u]);
        a.albedo = (const float4*)d_albedo;
        a.color = (const float4*)d_color;
        a.width = (int)width, a.height = (int)height, a.step = 1 << level;
        a.kc = dp->k_color * (float)(1u << (2u * level));
        a.kn = dp->k_normal, a.kd = dp->k_depth;
        a.flags = flags | (last ? DN_LAST : 0u);
        const uint32_t step = 1u << level;
        const bool lds = step <= kLdsMaxStep && (form == 2 || (form == 0 && step <= kAutoLdsMaxStep));
        if (lds) {
            const dim3 grid((width + kTileW - 1u) / kTileW, (height + kTileRows * kLdsPixels - 1u) / (kTileRows * kLdsPixels));
            const size_t bytes = lds_bytes(step, guide);
            if (guide)
                hipLaunchKernelGGL(dn_level_lds_kernel<true>, grid, dim3(kDnBlock), bytes, stream, a);
            else
                hipLaunchKernelGGL(dn_level_lds_kernel<false>, grid, dim3(kDnBlock), bytes, stream, a);
        } else {
            const dim3 grid((width + kTileW - 1u) / kTileW, (height + kTileRows - 1u) / kTileRows);
            if (guide)
                hipLaunchKernelGGL(dn_level_direct_kernel<true>, grid, dim3(kDnBlock), 0, stream, a);
            else
                hipLaunchKernelGGL(dn_level_direct_kernel<false>, grid, dim3(kDnBlock), 0, stream, a);
        }
        e = hipGetLastError();
        if (e != hipSuccess) {
            set_err(err, errlen, "denoise level launch", e);
            return -1;
        }
    }
    return 0;
}

extern "C" int wo_dev_denoise_work_begin(int device, size_t frame_pixels, size_t pixels, size_t scratch_bytes,
                                         WoDenoiseWork* work, char* err, size_t errlen) {
    memset(work, 0, sizeof *work);
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) {
        set_err(err, errlen, "hipSetDevice", e);
        return -1;
    }
    const size_t plane = pixels * sizeof(float4), frame = frame_pixels * sizeof(float4);
    e = hipMalloc(&work->base, frame + 4u * plane + scratch_bytes);
    if (e != hipSuccess) {
        work->base = nullptr;
        set_err(err, errlen, "hipMalloc(denoise buffers)", e);
        return -1;
    }
    char* b = (char*)work->base;
    work->d_color = b;
    work->d_planes = b + frame;
    work->d_out = b + frame + 3u * plane;
    work->d_scratch = b + frame + 4u * plane;
    return 0;
}

extern "C" int wo_dev_denoise_work_finish(WoDenoiseWork* work, void* host, size_t bytes, char* err, size_t errlen) {
    hipError_t e = hipMemcpyAsync(host, work->d_out, bytes, hipMemcpyDeviceToHost, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    wo_dev_denoise_work_free(work);
    if (e != hipSuccess) {
        set_err(err, errlen, "denoised frame (device->host)", e);
        return -1;
    }
    return 0;
}

extern "C" void wo_dev_denoise_work_free(WoDenoiseWork* work) {
    if (work->base) {
        (void)hipStreamSynchronize(nullptr);
        (void)hipFree(work->base);
    }
    memset(work, 0, sizeof *work);
}
