/* Stand-alone driver of csrc/mesh.c (make -C csgrenderer_amd/csrc mesh-asan builds it with
 * ASan + UBSan): wo_mesh_grid_check, wo_mesh_scratch_bytes and the device form's argument
 * checks over a table of good and bad grids and argument sets, wo_mesh_free, and the OBJ
 * writer on a small hand-made mesh whose arrays sit between guard bytes.  argv[1]: a directory
 * to write the OBJ files to.  Exit status 0 and "mesh driver: ok" when every check holds. */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wo_internal.h"

static char g_error[256];
static int g_failed;

void wo_set_error(char const* fmt, ...) { /* renderer.c's, for a program without the renderer */
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

static Wo_MeshGrid grid(float lo, float hi, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t iters) {
    Wo_MeshGrid g;
    memset(&g, 0, sizeof g);
    for (int a = 0; a < 3; ++a) g.lo[a] = lo, g.hi[a] = hi;
    g.n[0] = n0, g.n[1] = n1, g.n[2] = n2, g.iters = iters;
    return g;
}

static void good_grids(void) {
    float h[3];
    Wo_MeshGrid g = grid(-2.0f, 2.0f, 32, 16, 2, 16);
    CHECK(wo_mesh_grid_check(&g, h) == 0 && h[0] == 0.125f && h[1] == 0.25f && h[2] == 2.0f, "dyadic grid: %s", g_error);
    CHECK(wo_mesh_grid_check(&g, NULL) == 0, "NULL h_out: %s", g_error);
    /* 33 * 17 * 3 = 1683 corners: 27 words, 1 chunk */
    const WoMeshLayout l = wo_mesh_layout(g.n);
    CHECK(l.corners == 1683 && l.words == 27 && l.chunks == 1, "layout %llu %llu %llu", (unsigned long long)l.corners,
          (unsigned long long)l.words, (unsigned long long)l.chunks);
    CHECK(l.bits_off == 0 && l.masks_off == 27 * 8 && l.wcnt_off == 27 * 40 && l.chunks_off == 27 * 48 &&
              l.cross_off == 27 * 48 + 16 && l.bytes == l.cross_off + ((1683u * 12u + 15u) & ~15u),
          "layout offsets");
    CHECK(wo_mesh_scratch_bytes(&g) == l.bytes, "scratch bytes");
    g = grid(-1e30f, 1e30f, 1024, 1024, 1024, 24);
    CHECK(wo_mesh_grid_check(&g, h) == 0 && h[0] == 2e30f / 1024.0f, "largest grid: %s", g_error);
    const WoMeshLayout big = wo_mesh_layout(g.n);
    CHECK(big.corners == 1025ull * 1025ull * 1025ull && big.corners < (1ull << 31) && big.corners * 3u < (1ull << 32),
          "largest grid's corners");
    CHECK(wo_mesh_scratch_bytes(&g) == big.bytes && big.bytes > big.corners * 12u, "largest grid's scratch");
    g = grid(0.0f, 1.0f, 2, 2, 2, 0);
    CHECK(wo_mesh_grid_check(&g, h) == 0 && h[0] == 0.5f, "smallest grid: %s", g_error);
    g = grid(1.0f, nextafterf(1.0f, 2.0f), 2, 3, 1000, 3); /* h = 2^-24, 2^-23 / 3, 2^-23 / 1000: positive */
    CHECK(wo_mesh_grid_check(&g, h) == 0 && h[0] == 0x1p-24f && h[2] > 0.0f, "one-ulp box: %s", g_error);
}

static void bad_grids(void) {
    const Wo_MeshGrid ok = grid(-1.0f, 1.0f, 4, 4, 4, 8);
    struct {
        Wo_MeshGrid g;
        const char* text;
    } bad[16];
    int n = 0;
    for (int i = 0; i < 16; ++i) bad[i].g = ok;
    bad[n].g.lo[0] = NAN, bad[n++].text = "not finite";
    bad[n].g.hi[2] = INFINITY, bad[n++].text = "not finite";
    bad[n].g.lo[1] = 1.0f, bad[n++].text = "lo < hi";
    bad[n].g.hi[2] = -2.0f, bad[n++].text = "lo < hi";
    bad[n].g.n[0] = 1, bad[n++].text = "cells on axis 0";
    bad[n].g.n[1] = 0, bad[n++].text = "cells on axis 1";
    bad[n].g.n[2] = 1025, bad[n++].text = "cells on axis 2";
    bad[n].g.iters = 25, bad[n++].text = "bisection steps";
    bad[n].g.flags = 1, bad[n++].text = "flags";
    bad[n].g.reserved = 7, bad[n++].text = "reserved";
    bad[n].g.lo[0] = -3e38f, bad[n].g.hi[0] = 3e38f, bad[n++].text = "cell size"; /* the extent overflows */
    bad[n].g.lo[0] = 0.0f, bad[n].g.hi[0] = 0x1p-149f, bad[n++].text = "cell size"; /* h underflows to 0 */
    /* the order: the first failing check is named */
    bad[n].g.lo[0] = NAN, bad[n].g.n[0] = 0, bad[n].g.reserved = 1, bad[n++].text = "not finite";
    bad[n].g.n[0] = 0, bad[n].g.iters = 99, bad[n].g.flags = 1, bad[n++].text = "cells on axis 0";
    bad[n].g.iters = 99, bad[n].g.flags = 1, bad[n].g.reserved = 1, bad[n++].text = "bisection steps";
    bad[n].g.flags = 1, bad[n].g.reserved = 1, bad[n++].text = "flags";
    float h[3] = {-1.0f, -1.0f, -1.0f};
    for (int i = 0; i < n; ++i) {
        g_error[0] = 0;
        CHECK(wo_mesh_grid_check(&bad[i].g, h) == -1 && strstr(g_error, bad[i].text) && strstr(g_error, "mesh grid"),
              "bad grid %d: '%s' does not name '%s'", i, g_error, bad[i].text);
        CHECK(h[0] == -1.0f, "bad grid %d wrote h", i);
        CHECK(wo_mesh_scratch_bytes(&bad[i].g) == 0, "bad grid %d has a scratch size", i);
    }
    g_error[0] = 0;
    CHECK(wo_mesh_grid_check(NULL, h) == -1 && strstr(g_error, "NULL grid"), "NULL grid: %s", g_error);
    CHECK(wo_mesh_scratch_bytes(NULL) == 0, "NULL grid has a scratch size");
}

static void argument_checks(void) {
    const Wo_MeshGrid ok = grid(-1.0f, 1.0f, 4, 5, 6, 8);
    const size_t need = wo_mesh_scratch_bytes(&ok);
    /* addresses only: the checks never read through them */
    void *v = (void*)0x10000, *q = (void*)0x20000, *ids = (void*)0x30000, *c = (void*)0x40000, *s = (void*)0x50000;
    WoMeshLaunch ml;
    CHECK(wo_mesh_args_check(&ok, v, 10, q, ids, 20, c, s, need, &ml) == 0, "good arguments: %s", g_error);
    CHECK(ml.n[0] == 4 && ml.n[1] == 5 && ml.n[2] == 6 && ml.iters == 8 && ml.max_vertices == 10 && ml.max_quads == 20 &&
              ml.lo[1] == -1.0f && ml.h[0] == 0.5f && ml.h[1] == 2.0f / 5.0f,
          "the launch");
    CHECK(wo_mesh_args_check(&ok, NULL, 0, NULL, NULL, 0, c, s, need + 1000, &ml) == 0 && ml.max_vertices == 0 &&
              ml.max_quads == 0,
          "counts only: %s", g_error);
    CHECK(wo_mesh_args_check(&ok, v, 10, q, NULL, 20, c, s, need, NULL) == 0, "no ids, no launch: %s", g_error);
#define REFUSED(text, ...)                                                                            \
    do {                                                                                              \
        g_error[0] = 0;                                                                               \
        CHECK(wo_mesh_args_check(__VA_ARGS__) == -1 && strstr(g_error, text), "'%s' does not name '%s'", g_error, text); \
    } while (0)
    Wo_MeshGrid bad = ok;
    bad.iters = 25;
    REFUSED("bisection steps", &bad, NULL, 10, NULL, NULL, 20, NULL, NULL, 0, &ml); /* the grid comes first */
    REFUSED("NULL counts", &ok, NULL, 10, q, ids, 20, NULL, NULL, 0, &ml);
    REFUSED("NULL scratch", &ok, NULL, 10, q, ids, 20, c, NULL, 0, &ml);
    REFUSED("NULL vertex", &ok, NULL, 10, NULL, ids, 20, c, s, 0, &ml);
    REFUSED("NULL quad", &ok, v, 10, NULL, ids, 20, c, (char*)s + 4, 0, &ml);
    REFUSED("16-byte aligned", &ok, (char*)v + 8, 10, q, ids, 20, c, s, 0, &ml);
    REFUSED("16-byte aligned", &ok, v, 10, (char*)q + 4, ids, 20, c, s, need, &ml);
    REFUSED("16-byte aligned", &ok, v, 10, q, (char*)ids + 1, 20, c, s, need, &ml);
    REFUSED("16-byte aligned", &ok, v, 10, q, ids, 20, (char*)c + 8, s, need, &ml);
    REFUSED("16-byte aligned", &ok, v, 10, q, ids, 20, c, (char*)s + 8, need, &ml);
    REFUSED("short of", &ok, v, 10, q, ids, 20, c, s, need - 1, &ml);
    REFUSED("short of", &ok, NULL, 0, NULL, NULL, 0, c, s, 0, &ml);
#undef REFUSED
}

/* a copy of `bytes` bytes between two 64-byte guards of 0xA5; ASan watches the rest */
static void* guarded(void const* src, size_t bytes, unsigned char** block) {
    *block = (unsigned char*)malloc(bytes + 128u);
    memset(*block, 0xA5, bytes + 128u);
    if (bytes) memcpy(*block + 64, src, bytes);
    return *block + 64;
}
static int guards_intact(unsigned char const* block, size_t bytes) {
    for (size_t i = 0; i < 64; ++i)
        if (block[i] != 0xA5 || block[64 + bytes + i] != 0xA5) return 0;
    return 1;
}

static void obj_writer(const char* dir) {
    /* a unit cube: 8 vertices, 6 quads of nodes 7, 3, 7, cap, 3, cap */
    Wo_MeshVertex v[8];
    for (uint32_t i = 0; i < 8; ++i) {
        v[i].p[0] = (float)(i & 1u) + 0.1f, v[i].p[1] = (float)((i >> 1) & 1u) / 3.0f, v[i].p[2] = (float)(i >> 2) * 1e-8f;
        v[i].cell = i;
    }
    const Wo_MeshQuad q[6] = {{{0, 2, 3, 1}}, {{4, 5, 7, 6}}, {{0, 1, 5, 4}}, {{2, 6, 7, 3}}, {{0, 4, 6, 2}}, {{1, 3, 7, 5}}};
    const uint32_t node[6] = {7, 3, 7, 0xFFFFFFFFu, 3, 0xFFFFFFFFu};
    Wo_MeshQuadIds ids[6];
    for (int i = 0; i < 6; ++i) {
        ids[i].leaf = node[i] == 0xFFFFFFFFu ? node[i] : 10u + (uint32_t)i;
        ids[i].node = node[i], ids[i].material = node[i] == 0xFFFFFFFFu ? node[i] : 0u;
        ids[i].flags = (uint32_t)(i % 3) | (node[i] == 0xFFFFFFFFu ? WO_MESH_QUAD_CAP : 0u);
    }
    unsigned char *bv, *bq, *bi;
    Wo_MeshVertex* gv = (Wo_MeshVertex*)guarded(v, sizeof v, &bv);
    Wo_MeshQuad* gq = (Wo_MeshQuad*)guarded(q, sizeof q, &bq);
    Wo_MeshQuadIds* gi = (Wo_MeshQuadIds*)guarded(ids, sizeof ids, &bi);
    char path[1024], line[256];
    snprintf(path, sizeof path, "%s/mesh_driver_ids.obj", dir);
    CHECK(wo_mesh_write_obj(path, gv, 8, gq, gi, 6) == 0, "write with ids: %s", g_error);
    /* the groups in ascending node order, then the caps; quad order kept inside a group */
    const char* want[] = {"g node_3", "f 5 6 8 7", "f 1 5 7 3", "g node_7", "f 1 3 4 2", "f 1 2 6 5",
                          "g cap",    "f 3 7 8 4", "f 2 4 8 6"};
    FILE* fh = fopen(path, "r");
    CHECK(fh != NULL, "cannot read %s back", path);
    if (fh) {
        int nv = 0, k = 0;
        while (fgets(line, sizeof line, fh)) {
            line[strcspn(line, "\n")] = 0;
            if (line[0] == 'v') {
                float x, y, z;
                CHECK(sscanf(line + 2, "%f %f %f", &x, &y, &z) == 3 && x == v[nv].p[0] && y == v[nv].p[1] && z == v[nv].p[2],
                      "vertex %d does not round-trip: %s", nv, line);
                ++nv;
            } else if (line[0] == 'g' || line[0] == 'f') {
                CHECK(k < 9 && strcmp(line, want[k]) == 0, "line %d is '%s'", k, line);
                ++k;
            }
        }
        CHECK(nv == 8 && k == 9, "%d vertices, %d group and face lines", nv, k);
        fclose(fh);
    }
    snprintf(path, sizeof path, "%s/mesh_driver_plain.obj", dir);
    CHECK(wo_mesh_write_obj(path, gv, 8, gq, NULL, 6) == 0, "write without ids: %s", g_error);
    CHECK(wo_mesh_write_obj(path, NULL, 0, NULL, NULL, 0) == 0, "the empty mesh: %s", g_error);
    CHECK(wo_mesh_write_obj(path, gv, 7, gq, gi, 6) == -1 && strstr(g_error, "names vertex"), "a quad past the vertices: %s",
          g_error);
    CHECK(wo_mesh_write_obj(NULL, gv, 8, gq, gi, 6) == -1 && wo_mesh_write_obj(path, NULL, 8, gq, gi, 6) == -1 &&
              wo_mesh_write_obj(path, gv, 8, NULL, gi, 6) == -1,
          "NULL was accepted");
    snprintf(path, sizeof path, "%s/no/such/directory/mesh.obj", dir);
    CHECK(wo_mesh_write_obj(path, gv, 8, gq, gi, 6) == -1 && strstr(g_error, "cannot open"), "a bad path: %s", g_error);
    CHECK(guards_intact(bv, sizeof v) && guards_intact(bq, sizeof q) && guards_intact(bi, sizeof ids), "a guard was written");
    CHECK(memcmp(gv, v, sizeof v) == 0 && memcmp(gq, q, sizeof q) == 0 && memcmp(gi, ids, sizeof ids) == 0,
          "an input was written");
    free(bv), free(bq), free(bi);

    Wo_Mesh m;
    memset(&m, 0, sizeof m);
    m.vertices = (Wo_MeshVertex*)malloc(sizeof v), m.quads = (Wo_MeshQuad*)malloc(sizeof q);
    m.quad_ids = NULL, m.counts.vertices = 8, m.counts.quads = 6;
    wo_mesh_free(&m);
    CHECK(!m.vertices && !m.quads && !m.quad_ids && m.counts.vertices == 0 && m.counts.quads == 0, "wo_mesh_free left something");
    wo_mesh_free(&m); /* twice, and NULL */
    wo_mesh_free(NULL);
}

int main(int argc, char** argv) {
    good_grids();
    bad_grids();
    argument_checks();
    obj_writer(argc > 1 ? argv[1] : ".");
    if (g_failed) {
        printf("mesh driver: %d checks failed\n", g_failed);
        return 1;
    }
    printf("mesh driver: ok\n");
    return 0;
}
