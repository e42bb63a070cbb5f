/*
 * mesh.c -- the host side of the surface-mesh query (renderer_ext.h Wo_MeshGrid): the grid
 * check and the cell sizes host and kernels share, the scratch size, the device form's
 * argument checks, the OBJ writer and wo_mesh_free.  Host only, no HIP:
 * tests/host/mesh_main.c drives it under ASan + UBSan (make mesh-asan).
 */
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wo_internal.h"

_Static_assert(sizeof(Wo_MeshGrid) == 48 && sizeof(Wo_MeshVertex) == 16 && sizeof(Wo_MeshQuad) == 16 &&
                   sizeof(Wo_MeshQuadIds) == 16 && sizeof(Wo_MeshCounts) == 16,
               "the mesh's rows are 16 bytes, Wo_MeshGrid 48");

int wo_mesh_grid_check(Wo_MeshGrid const* g, float h_out[3]) {
    if (!g) {
        wo_set_error("mesh grid: NULL grid");
        return -1;
    }
    for (int a = 0; a < 3; ++a)
        if (!isfinite(g->lo[a]) || !isfinite(g->hi[a])) {
            wo_set_error("mesh grid: clip box is not finite on axis %d", a);
            return -1;
        }
    for (int a = 0; a < 3; ++a)
        if (!(g->lo[a] < g->hi[a])) {
            wo_set_error("mesh grid: clip box needs lo < hi on axis %d (%g, %g)", a, (double)g->lo[a], (double)g->hi[a]);
            return -1;
        }
    for (int a = 0; a < 3; ++a)
        if (g->n[a] < 2u || g->n[a] > WO_MESH_MAX_CELLS) {
            wo_set_error("mesh grid: %u cells on axis %d (2 .. %u)", g->n[a], a, WO_MESH_MAX_CELLS);
            return -1;
        }
    if (g->iters > WO_MESH_MAX_ITERS) {
        wo_set_error("mesh grid: %u bisection steps (0 .. %u)", g->iters, WO_MESH_MAX_ITERS);
        return -1;
    }
    if (g->flags != 0u) {
        wo_set_error("mesh grid: flags must be 0 (none is defined)");
        return -1;
    }
    if (g->reserved != 0u) {
        wo_set_error("mesh grid: reserved must be 0");
        return -1;
    }
    float h[3];
    for (int a = 0; a < 3; ++a) {
        const float extent = g->hi[a] - g->lo[a];
        h[a] = extent / (float)g->n[a];
        if (!isfinite(h[a]) || !(h[a] > 0.0f)) {
            wo_set_error("mesh grid: the cell size on axis %d is not a positive finite fp32 (%g)", a, (double)h[a]);
            return -1;
        }
    }
    if (h_out) memcpy(h_out, h, sizeof h);
    return 0;
}

size_t wo_mesh_scratch_bytes(Wo_MeshGrid const* g) {
    if (wo_mesh_grid_check(g, NULL)) return 0;
    return wo_mesh_layout(g->n).bytes;
}

int wo_mesh_args_check(Wo_MeshGrid const* g, void const* d_vertices, uint32_t max_vertices, void const* d_quads,
                       void const* d_quad_ids, uint32_t max_quads, void const* d_counts, void const* d_scratch,
                       size_t scratch_bytes, WoMeshLaunch* ml) {
    float h[3];
    if (wo_mesh_grid_check(g, h)) return -1;
    if (!d_counts || !d_scratch) {
        wo_set_error("mesh: NULL %s buffer", !d_counts ? "counts" : "scratch");
        return -1;
    }
    if ((max_vertices != 0u && !d_vertices) || (max_quads != 0u && !d_quads)) {
        wo_set_error("mesh: NULL %s buffer with a maximum of %u rows", max_vertices != 0u && !d_vertices ? "vertex" : "quad",
                     max_vertices != 0u && !d_vertices ? max_vertices : max_quads);
        return -1;
    }
    if (((uintptr_t)d_vertices | (uintptr_t)d_quads | (uintptr_t)d_quad_ids | (uintptr_t)d_counts | (uintptr_t)d_scratch) &
        15u) {
        wo_set_error("mesh: the vertex, quad, id, counts and scratch buffers must be 16-byte aligned");
        return -1;
    }
    const size_t need = wo_mesh_layout(g->n).bytes;
    if (scratch_bytes < need) {
        wo_set_error("mesh: %zu bytes of scratch are short of the %zu the grid needs (wo_mesh_scratch_bytes)",
                     scratch_bytes, need);
        return -1;
    }
    if (ml) {
        for (int a = 0; a < 3; ++a) {
            ml->lo[a] = g->lo[a];
            ml->h[a] = h[a];
            ml->n[a] = g->n[a];
        }
        ml->iters = g->iters;
        ml->max_vertices = d_vertices ? max_vertices : 0u;
        ml->max_quads = d_quads ? max_quads : 0u;
    }
    return 0;
}

void wo_mesh_free(Wo_Mesh* mesh) {
    if (!mesh) return;
    free(mesh->vertices);
    free(mesh->quads);
    free(mesh->quad_ids);
    memset(mesh, 0, sizeof *mesh);
}

static int cmp_u64(void const* a, void const* b) {
    const uint64_t x = *(uint64_t const*)a, y = *(uint64_t const*)b;
    return x < y ? -1 : x > y;
}

static int write_face(FILE* fh, Wo_MeshQuad const* q) {
    return fprintf(fh, "f %u %u %u %u\n", q->v[0] + 1u, q->v[1] + 1u, q->v[2] + 1u, q->v[3] + 1u) < 0 ? -1 : 0;
}

int wo_mesh_write_obj(char const* path, Wo_MeshVertex const* vertices, uint32_t n_vertices, Wo_MeshQuad const* quads,
                      Wo_MeshQuadIds const* ids, uint32_t n_quads) {
    if (!path || (n_vertices != 0u && !vertices) || (n_quads != 0u && !quads)) {
        wo_set_error("mesh obj: NULL path, vertices or quads");
        return -1;
    }
    for (uint32_t i = 0; i < n_quads; ++i)
        for (int c = 0; c < 4; ++c)
            if (quads[i].v[c] >= n_vertices) {
                wo_set_error("mesh obj: quad %u names vertex %u of %u (a truncated mesh cannot be written)", i,
                             quads[i].v[c], n_vertices);
                return -1;
            }
    /* with ids: the quads by (group, index); a group is a node id, the caps' 0xFFFFFFFF comes last by value */
    uint64_t* order = NULL;
    if (ids && n_quads != 0u) {
        order = (uint64_t*)malloc((size_t)n_quads * sizeof *order);
        if (!order) {
            wo_set_error("mesh obj: out of memory");
            return -1;
        }
        for (uint32_t i = 0; i < n_quads; ++i) {
            const uint32_t group = (ids[i].flags & WO_MESH_QUAD_CAP) != 0u ? WO_NODE_INVALID : ids[i].node;
            order[i] = (uint64_t)group << 32 | i;
        }
        qsort(order, n_quads, sizeof *order, cmp_u64);
    }
    FILE* fh = fopen(path, "w");
    if (!fh) {
        wo_set_error("mesh obj: cannot open %s: %s", path, strerror(errno));
        free(order);
        return -1;
    }
    int bad = fprintf(fh, "# %u vertices, %u quads\n", n_vertices, n_quads) < 0;
    for (uint32_t i = 0; i < n_vertices && !bad; ++i)
        bad = fprintf(fh, "v %.9g %.9g %.9g\n", (double)vertices[i].p[0], (double)vertices[i].p[1],
                      (double)vertices[i].p[2]) < 0;
    if (!ids) {
        for (uint32_t i = 0; i < n_quads && !bad; ++i) bad = write_face(fh, &quads[i]);
    } else {
        for (uint32_t k = 0; k < n_quads && !bad; ++k) {
            const uint32_t group = (uint32_t)(order[k] >> 32), i = (uint32_t)order[k];
            if (k == 0u || group != (uint32_t)(order[k - 1u] >> 32))
                bad = (group == WO_NODE_INVALID ? fprintf(fh, "g cap\n") : fprintf(fh, "g node_%u\n", group)) < 0;
            if (!bad) bad = write_face(fh, &quads[i]);
        }
    }
    free(order);
    if (fclose(fh) != 0) bad = 1;
    if (bad) {
        wo_set_error("mesh obj: writing %s failed", path);
        return -1;
    }
    return 0;
}
