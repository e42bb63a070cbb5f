/*
 * denoise.c -- the host side of the a-trous denoiser (renderer_ext.h wo_denoise_*): the
 * defaults, the argument checks that the device entry points share, the scratch size, and
 * the filter itself in host C, operation by operation as the header states it (and as
 * denoise_kernels.hip runs it: the two agree bit for bit).  Host only, no HIP:
 * tests/host/denoise_main.c drives it under ASan + UBSan (make denoise-asan).
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "wo_denoise.h"
#include "wo_internal.h"

_Static_assert(sizeof(Wo_DenoiseParams) == 24, "Wo_DenoiseParams is 24 bytes");

#define DN_KNOWN_FLAGS (WO_DENOISE_DEMODULATE | WO_DENOISE_STOP_AT_NODES)

void wo_denoise_params_default(Wo_DenoiseParams* dp) {
    if (!dp) return;
    memset(dp, 0, sizeof *dp);
    dp->levels = 5u;
    dp->flags = WO_DENOISE_DEMODULATE;
    dp->k_color = 0.25f;
    dp->k_normal = 4.0f;
    dp->k_depth = 100.0f;
}

int wo_denoise_check_params(char const* what, Wo_DenoiseParams const* dp) {
    if (!dp) {
        wo_set_error("%s: NULL params", what);
        return -1;
    }
    if (dp->levels < 1u || dp->levels > WO_DENOISE_MAX_LEVELS) {
        wo_set_error("%s: levels %u (1 .. %u)", what, dp->levels, WO_DENOISE_MAX_LEVELS);
        return -1;
    }
    if (dp->flags & ~DN_KNOWN_FLAGS) {
        wo_set_error("%s: unknown flags 0x%x", what, dp->flags & ~DN_KNOWN_FLAGS);
        return -1;
    }
    if (dp->reserved != 0u) {
        wo_set_error("%s: reserved must be 0", what);
        return -1;
    }
    const float k[3] = {dp->k_color, dp->k_normal, dp->k_depth};
    static char const* const name[3] = {"k_color", "k_normal", "k_depth"};
    for (int i = 0; i < 3; ++i)
        if (!isfinite(k[i]) || k[i] < 0.0f) {
            wo_set_error("%s: %s = %g (finite and >= 0)", what, name[i], (double)k[i]);
            return -1;
        }
    return 0;
}

int wo_denoise_check_extent(char const* what, uint32_t width, uint32_t height) {
    if (width == 0u || width > WO_DENOISE_MAX_EXTENT || height == 0u || height > WO_DENOISE_MAX_EXTENT) {
        wo_set_error("%s: width x height = %u x %u (1 .. %u each)", what, width, height, WO_DENOISE_MAX_EXTENT);
        return -1;
    }
    return 0;
}

static size_t scratch_bytes_of(uint32_t width, uint32_t height, Wo_DenoiseParams const* dp) {
    return (size_t)width * height * 16u * (dp->levels > 1u ? 2u : 1u);
}

static int overlaps(void const* a, size_t na, void const* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb ? pb - pa < na : pa - pb < nb;
}

int wo_denoise_check_planes(char const* what, Wo_DenoiseParams const* dp, uint32_t width, uint32_t height,
                            void const* color, void const* albedo, void const* normal, void const* ids, void const* out,
                            void const* scratch, size_t scratch_bytes, int device) {
    const int need_albedo = (dp->flags & WO_DENOISE_DEMODULATE) != 0u;
    const int need_normal = dp->k_normal > 0.0f || dp->k_depth > 0.0f;
    const int need_ids = (dp->flags & WO_DENOISE_STOP_AT_NODES) != 0u;
    void const* const in[4] = {color, albedo, normal, ids};
    static char const* const in_name[4] = {"color", "albedo", "normal", "ids"};
    const int need[4] = {1, need_albedo, need_normal, need_ids};
    static char const* const why[4] = {"", " (WO_DENOISE_DEMODULATE)", " (k_normal or k_depth > 0)",
                                       " (WO_DENOISE_STOP_AT_NODES)"};
    for (int i = 0; i < 4; ++i)
        if (need[i] && !in[i]) {
            wo_set_error("%s: the %s plane is NULL%s", what, in_name[i], why[i]);
            return -1;
        }
    if (!out) {
        wo_set_error("%s: the out plane is NULL", what);
        return -1;
    }
    if (device && !scratch) {
        wo_set_error("%s: the scratch buffer is NULL", what);
        return -1;
    }
    for (int i = 0; i < 4; ++i)
        if ((uintptr_t)in[i] & 15u) {
            wo_set_error("%s: the %s plane is not 16-byte aligned", what, in_name[i]);
            return -1;
        }
    if ((uintptr_t)out & 15u) {
        wo_set_error("%s: the out plane is not 16-byte aligned", what);
        return -1;
    }
    if (device && ((uintptr_t)scratch & 15u)) {
        wo_set_error("%s: the scratch buffer is not 16-byte aligned", what);
        return -1;
    }
    const size_t plane = (size_t)width * height * 16u, want = scratch_bytes_of(width, height, dp);
    for (int i = 0; i < 4; ++i)
        if (in[i] && overlaps(out, plane, in[i], plane)) {
            wo_set_error("%s: out overlaps the %s plane (aliasing)", what, in_name[i]);
            return -1;
        }
    for (int i = 0; i < 4; ++i)
        if (device && in[i] && overlaps(scratch, want, in[i], plane)) {
            wo_set_error("%s: scratch overlaps the %s plane (aliasing)", what, in_name[i]);
            return -1;
        }
    if (device && overlaps(scratch, want, out, plane)) {
        wo_set_error("%s: scratch overlaps out (aliasing)", what);
        return -1;
    }
    if (device && scratch_bytes < want) {
        wo_set_error("%s: scratch of %zu bytes is short of the %zu that wo_denoise_scratch_bytes asks for", what,
                     scratch_bytes, want);
        return -1;
    }
    return 0;
}

size_t wo_denoise_scratch_bytes(uint32_t width, uint32_t height, Wo_DenoiseParams const* dp) {
    if (wo_denoise_check_params("denoise_scratch_bytes", dp)) return 0u;
    if (wo_denoise_check_extent("denoise_scratch_bytes", width, height)) return 0u;
    return scratch_bytes_of(width, height, dp);
}

/* ---- the filter (renderer_ext.h; every line one fp32 operation, -ffp-contract=off) ---- */

static float clampf(float v, float lo, float hi) {
    const float t = v > lo ? v : lo;
    return t < hi ? t : hi;
}

static float edge(float d2, float k) {
    const float p = d2 * k;
    const float x = 1.0f - p;
    const float m = x > 0.0f ? x : 0.0f;
    return m * m;
}

static float dist2(float const* a, float const* b) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float s = xx + yy;
    return s + zz;
}

int wo_denoise_host(Wo_DenoiseParams const* dp, uint32_t width, uint32_t height, void const* color_v,
                    void const* albedo_v, void const* normal_v, void const* ids_v, void* out_v) {
    static char const what[] = "denoise_host";
    if (wo_denoise_check_params(what, dp)) return -1;
    if (wo_denoise_check_extent(what, width, height)) return -1;
    if (wo_denoise_check_planes(what, dp, width, height, color_v, albedo_v, normal_v, ids_v, out_v, NULL, 0u, 0)) return -1;
    const size_t n = (size_t)width * height;
    float const* color = (float const*)color_v;
    float const* albedo = (float const*)albedo_v;
    float const* normal = (float const*)normal_v;
    Wo_FeatureIds const* ids = (Wo_FeatureIds const*)ids_v;
    float* out = (float*)out_v;
    const int demod = (dp->flags & WO_DENOISE_DEMODULATE) != 0u, stop = (dp->flags & WO_DENOISE_STOP_AT_NODES) != 0u;
    const int on_color = dp->k_color > 0.0f, on_normal = dp->k_normal > 0.0f, on_depth = dp->k_depth > 0.0f;
    /* the working image and its successor (3 floats per pixel), the demodulation's a' */
    float* cur = (float*)malloc(n * 3u * sizeof(float));
    float* nxt = (float*)malloc(n * 3u * sizeof(float));
    float* amod = demod ? (float*)malloc(n * 3u * sizeof(float)) : NULL;
    if (!cur || !nxt || (demod && !amod)) {
        free(cur), free(nxt), free(amod);
        wo_set_error("%s: out of memory for a %u x %u working image", what, width, height);
        return -1;
    }
    for (size_t p = 0; p < n; ++p)
        for (int i = 0; i < 3; ++i) {
            if (demod) {
                const float a = clampf(albedo[4u * p + i], 0x1p-7f, 0x1p20f);
                const float ra = 1.0f / a;
                amod[3u * p + i] = a;
                cur[3u * p + i] = color[4u * p + i] * ra;
            } else {
                cur[3u * p + i] = color[4u * p + i];
            }
        }
    static const float H[3] = {0.375f, 0.25f, 0.0625f};
    const int W = (int)width, Hh = (int)height;
    for (uint32_t level = 0; level < dp->levels; ++level) {
        const int s = 1 << level;
        const float kc = dp->k_color * (float)(1u << (2u * level));
        for (int y = 0; y < Hh; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t p = (size_t)y * width + (size_t)x;
                float const* cp = cur + 3u * p;
                float const* np = normal ? normal + 4u * p : NULL;
                const float zp = np ? np[3] : 0.0f;
                const int finp = zp < INFINITY;
                const float rzp = on_depth ? 1.0f / clampf(zp, 0x1p-20f, 0x1p20f) : 0.0f;
                float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        const int qx = x + dx * s, qy = y + dy * s;
                        if (qx < 0 || qx >= W || qy < 0 || qy >= Hh) continue;
                        const size_t q = (size_t)qy * width + (size_t)qx;
                        float const* cq = cur + 3u * q;
                        const float h = H[abs(dx)] * H[abs(dy)];
                        float w = h;
                        if (dx != 0 || dy != 0) {
                            float e = 1.0f;
                            if (on_color) e *= edge(dist2(cq, cp), kc);
                            if (on_normal) e *= edge(dist2(normal + 4u * q, np), dp->k_normal);
                            if (on_depth) {
                                const float zq = normal[4u * q + 3u];
                                const int finq = zq < INFINITY;
                                if (finp && finq) {
                                    const float dz = zq - zp;
                                    const float rel = dz * rzp;
                                    e *= edge(rel * rel, dp->k_depth);
                                } else if (finp != finq) {
                                    e = 0.0f;
                                }
                            }
                            if (stop && ids[q].node != ids[p].node) e = 0.0f;
                            w = h * e;
                        }
                        if (!(w > 0.0f)) continue;
                        for (int i = 0; i < 3; ++i) {
                            const float t = w * cq[i];
                            sum[i] += t;
                        }
                        wsum += w;
                    }
                const float rw = 1.0f / wsum;
                for (int i = 0; i < 3; ++i) nxt[3u * p + i] = sum[i] * rw;
            }
        float* t = cur;
        cur = nxt;
        nxt = t;
    }
    for (size_t p = 0; p < n; ++p) {
        for (int i = 0; i < 3; ++i) out[4u * p + i] = demod ? cur[3u * p + i] * amod[3u * p + i] : cur[3u * p + i];
        memcpy(out + 4u * p + 3u, color + 4u * p + 3u, sizeof(float));
    }
    free(cur), free(nxt), free(amod);
    return 0;
}
