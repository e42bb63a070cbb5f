/* Stand-alone driver of csrc/denoise.c (make -C csgrenderer_amd/csrc denoise-asan builds it with
 * ASan + UBSan): the defaults, the scratch size, a table of good and bad argument sets through
 * the shared checks and wo_denoise_host, and the host filter on a small image whose every buffer
 * is an exact-size heap block (so the sanitizer's redzones guard both ends) with guard rows of
 * its own behind the output.  Exit status 0 and "denoise driver: ok" when every check holds. */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wololo/renderer/renderer_ext.h"

/* csrc/wo_denoise.h, for a program without the renderer */
int wo_denoise_check_params(char const* what, Wo_DenoiseParams const* dp);
int wo_denoise_check_extent(char const* what, uint32_t width, uint32_t height);
int wo_denoise_check_planes(char const* what, Wo_DenoiseParams const* dp, uint32_t width, uint32_t height,
                            void const* color, void const* albedo, void const* normal, void const* ids, void const* out,
                            void const* scratch, size_t scratch_bytes, int device);

static char g_error[512];
static int g_failed;

void wo_set_error(char const* fmt, ...) { /* renderer.c's */
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

#define CHECK(cond, ...)                                       \
    do {                                                       \
        if (!(cond)) {                                         \
            printf("FAILED %s:%d: ", __FILE__, __LINE__);      \
            printf(__VA_ARGS__);                               \
            printf("\n");                                      \
            ++g_failed;                                        \
        }                                                      \
    } while (0)

#define W 13u
#define H 9u
#define GUARD_ROWS 3u
#define SENTINEL 0xA5A5A5A5u

static float* plane(void) { /* exactly W * H rows: one byte further is the sanitizer's */
    float* p = (float*)aligned_alloc(16, (size_t)W * H * 16u);
    if (!p) abort();
    return p;
}

static uint32_t lcg(uint32_t* s) { return *s = *s * 1664525u + 1013904223u; }
static float unit(uint32_t* s) { return (float)(lcg(s) >> 8) * 0x1p-24f; }

static void defaults_and_scratch(void) {
    Wo_DenoiseParams dp;
    memset(&dp, 0xff, sizeof dp);
    wo_denoise_params_default(&dp);
    CHECK(dp.levels == 5u && dp.flags == WO_DENOISE_DEMODULATE && dp.k_color == 0.25f && dp.k_normal == 4.0f &&
              dp.k_depth == 100.0f && dp.reserved == 0u, "defaults");
    wo_denoise_params_default(NULL);
    CHECK(wo_denoise_scratch_bytes(W, H, &dp) == (size_t)W * H * 32u, "scratch of 5 levels");
    dp.levels = 1u;
    CHECK(wo_denoise_scratch_bytes(W, H, &dp) == (size_t)W * H * 16u, "scratch of 1 level");
    CHECK(wo_denoise_scratch_bytes(32768u, 32768u, &dp) == (size_t)1 << 34, "largest frame");
    CHECK(wo_denoise_scratch_bytes(0u, H, &dp) == 0u && wo_denoise_scratch_bytes(W, 32769u, &dp) == 0u &&
              wo_denoise_scratch_bytes(W, H, NULL) == 0u, "bad extents give 0");
    dp.levels = 9u;
    CHECK(wo_denoise_scratch_bytes(W, H, &dp) == 0u, "bad levels give 0");
}

static void bad_arguments(void) {
    Wo_DenoiseParams ok;
    wo_denoise_params_default(&ok);
    ok.flags |= WO_DENOISE_STOP_AT_NODES;
    float *color = plane(), *albedo = plane(), *normal = plane(), *ids = plane(), *out = plane();
    float* scratch = (float*)aligned_alloc(16, (size_t)W * H * 32u);
    if (!scratch) abort();
    const size_t sb = (size_t)W * H * 32u;
    /* in the header's order; each entry breaks one thing of a good call */
    struct {
        char const* word;
        int field; /* which thing */
    } const table[] = {{"NULL params", 0}, {"levels", 1}, {"levels", 2}, {"flags", 3}, {"reserved", 4}, {"k_color", 5},
                       {"k_normal", 6}, {"k_depth", 7}, {"width", 8}, {"width", 9}, {"color plane is NULL", 10},
                       {"albedo plane is NULL", 11}, {"normal plane is NULL", 12}, {"ids plane is NULL", 13},
                       {"out plane is NULL", 14}, {"scratch buffer is NULL", 15}, {"aligned", 16}, {"aligned", 17},
                       {"aligned", 18}, {"aliasing", 19}, {"aliasing", 20}, {"aliasing", 21}, {"short", 22}};
    for (size_t i = 0; i < sizeof table / sizeof table[0]; ++i) {
        Wo_DenoiseParams dp = ok;
        Wo_DenoiseParams const* dpp = &dp;
        uint32_t w = W, h = H;
        void const *c = color, *a = albedo, *n = normal, *d = ids, *o = out, *s = scratch;
        size_t bytes = sb;
        switch (table[i].field) {
        case 0: dpp = NULL; break;
        case 1: dp.levels = 0u; break;
        case 2: dp.levels = 9u; break;
        case 3: dp.flags |= 4u; break;
        case 4: dp.reserved = 1u; break;
        case 5: dp.k_color = -1.0f; break;
        case 6: dp.k_normal = NAN; break;
        case 7: dp.k_depth = INFINITY; break;
        case 8: w = 0u; break;
        case 9: h = 32769u; break;
        case 10: c = NULL; break;
        case 11: a = NULL; break;
        case 12: n = NULL; break;
        case 13: d = NULL; break;
        case 14: o = NULL; break;
        case 15: s = NULL; break;
        case 16: c = (char const*)color + 4; break;
        case 17: o = (char const*)out + 8; break;
        case 18: s = (char const*)scratch + 4; break;
        case 19: o = color; break;
        case 20: s = normal; break;
        case 21: s = (char const*)out + 16; break; /* overlapping, not equal */
        case 22: bytes = sb - 1u; break;
        default: break;
        }
        g_error[0] = 0;
        int rc = wo_denoise_check_params("driver", dpp);
        if (!rc) rc = wo_denoise_check_extent("driver", w, h);
        if (!rc) rc = wo_denoise_check_planes("driver", dpp, w, h, c, a, n, d, o, s, bytes, 1);
        CHECK(rc == -1 && strstr(g_error, table[i].word), "bad argument set %zu (%s): rc %d, \"%s\"", i, table[i].word, rc,
              g_error);
        if (table[i].field < 15 && table[i].field != 14) { /* the host form refuses it too, before it reads a plane */
            g_error[0] = 0;
            CHECK(wo_denoise_host(dpp, w, h, c, a, n, d, out) == -1 && strstr(g_error, table[i].word),
                  "host form, bad argument set %zu (%s): \"%s\"", i, table[i].word, g_error);
        }
    }
    /* optional planes may be NULL exactly when nothing reads them */
    Wo_DenoiseParams dp = ok;
    dp.flags = 0u, dp.k_normal = 0.0f, dp.k_depth = 0.0f;
    CHECK(wo_denoise_check_planes("driver", &dp, W, H, color, NULL, NULL, NULL, out, scratch, sb, 1) == 0, "%s", g_error);
    CHECK(wo_denoise_check_planes("driver", &ok, W, H, color, albedo, normal, ids, out, scratch, sb + 64u, 1) == 0, "%s", g_error);
    free(color), free(albedo), free(normal), free(ids), free(out), free(scratch);
}

static void filter_small_image(void) {
    uint32_t seed = 7u;
    float *color = plane(), *albedo = plane(), *normal = plane();
    Wo_FeatureIds* ids = (Wo_FeatureIds*)plane();
    uint32_t* out = (uint32_t*)aligned_alloc(16, (size_t)(W * H + GUARD_ROWS * W) * 16u);
    if (!out) abort();
    for (uint32_t p = 0; p < W * H; ++p) {
        const uint32_t block = (p % W) / 5u + 3u * ((p / W) / 4u);
        for (int i = 0; i < 3; ++i) {
            albedo[4u * p + i] = block == 2u ? 0.0f : 0.2f + 0.1f * (float)block;
            color[4u * p + i] = albedo[4u * p + i] * (0.5f + unit(&seed));
            normal[4u * p + i] = (i == (int)(block % 3u) ? 1.0f : 0.0f) + 0.1f * (unit(&seed) - 0.5f);
        }
        albedo[4u * p + 3u] = 1.0f;
        color[4u * p + 3u] = unit(&seed);
        normal[4u * p + 3u] = block == 4u ? INFINITY : 2.0f + (float)block + 0.05f * unit(&seed);
        ids[p].node = block, ids[p].leaf = block, ids[p].material = 0u, ids[p].flags = 1u;
    }
    color[4u * 17u + 1u] = NAN;
    color[4u * 80u + 0u] = INFINITY;
    for (uint32_t levels = 1u; levels <= WO_DENOISE_MAX_LEVELS; ++levels)
        for (uint32_t flags = 0u; flags < 4u; ++flags) {
            Wo_DenoiseParams dp;
            wo_denoise_params_default(&dp);
            dp.levels = levels, dp.flags = flags, dp.k_color = 1.0f;
            for (uint32_t i = 0; i < (W * H + GUARD_ROWS * W) * 4u; ++i) out[i] = SENTINEL;
            g_error[0] = 0;
            CHECK(wo_denoise_host(&dp, W, H, color, albedo, normal, ids, out) == 0, "levels %u flags %u: %s", levels, flags,
                  g_error);
            int guards = 1, alpha = 1, nonfinite = 0;
            for (uint32_t i = W * H * 4u; i < (W * H + GUARD_ROWS * W) * 4u; ++i) guards &= out[i] == SENTINEL;
            for (uint32_t p = 0; p < W * H; ++p) {
                alpha &= memcmp(&out[4u * p + 3u], &color[4u * p + 3u], 4u) == 0;
                float v[3];
                memcpy(v, &out[4u * p], sizeof v);
                nonfinite += !(isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]));
            }
            CHECK(guards, "levels %u flags %u: a guard row was written", levels, flags);
            CHECK(alpha, "levels %u flags %u: alpha is not the frame's", levels, flags);
            CHECK(nonfinite == 2, "levels %u flags %u: %d non-finite pixels (the NaN and the +inf pixel: 2)", levels, flags,
                  nonfinite);
        }
    /* only the colour plane, one pixel wide and one pixel high */
    Wo_DenoiseParams dp;
    wo_denoise_params_default(&dp);
    dp.flags = 0u, dp.k_normal = 0.0f, dp.k_depth = 0.0f, dp.levels = 8u;
    CHECK(wo_denoise_host(&dp, W * H, 1u, color, NULL, NULL, NULL, out) == 0, "%u x 1: %s", W * H, g_error);
    CHECK(wo_denoise_host(&dp, 1u, W * H, color, NULL, NULL, NULL, out) == 0, "1 x %u: %s", W * H, g_error);
    CHECK(wo_denoise_host(&dp, 1u, 1u, color, NULL, NULL, NULL, out) == 0, "1 x 1: %s", g_error);
    free(color), free(albedo), free(normal), free(ids), free(out);
}

int main(void) {
    defaults_and_scratch();
    bad_arguments();
    filter_small_image();
    if (g_failed) {
        printf("denoise driver: %d checks failed\n", g_failed);
        return 1;
    }
    printf("denoise driver: ok\n");
    return 0;
}
