/*
 * abi.c -- the C compiler's view of the value types that cross the C ABI
 * (renderer.h, renderer_ext.h, wo_scene.h), so bindings in other languages can
 * check their mirrors field by field (tests/test_api.py checks the ctypes ones
 * in csgrenderer_amd/wololo.py).  The reference passes Wo_Node_Argument by
 * value (renderer.h:22-33); a mirror with a wrong field offset corrupts every
 * binop silently, so the check is worth an exported symbol.
 */
#include <stddef.h>
#include <string.h>

#include "wololo/renderer/renderer_ext.h"
#include "wololo/wo_scene.h"

typedef struct AbiField {
    const char* type;
    const char* field; /* NULL: the type's size */
    size_t value;
} AbiField;

#define T(ty) {#ty, NULL, sizeof(ty)}
#define F(ty, fl) {#ty, #fl, offsetof(ty, fl)}

static const AbiField kAbi[] = {
    T(Wo_Vec3), F(Wo_Vec3, x), F(Wo_Vec3, y), F(Wo_Vec3, z),
    T(Wo_Quaternion), F(Wo_Quaternion, real), F(Wo_Quaternion, imaginary),
    T(Wo_Node_Argument), F(Wo_Node_Argument, orientation), F(Wo_Node_Argument, offset), F(Wo_Node_Argument, node),
    T(Wo_RenderParams), F(Wo_RenderParams, width), F(Wo_RenderParams, height), F(Wo_RenderParams, spp),
    F(Wo_RenderParams, max_depth), F(Wo_RenderParams, seed), F(Wo_RenderParams, mode),
    F(Wo_RenderParams, sample_offset), F(Wo_RenderParams, time_sec),
    T(WoRec), F(WoRec, op), F(WoRec, u0), F(WoRec, u1), F(WoRec, f),
    T(WoMaterial), F(WoMaterial, kind), F(WoMaterial, albedo), F(WoMaterial, fuzz), F(WoMaterial, ior),
    F(WoMaterial, inv_ior), F(WoMaterial, r0),
    T(WoCamera), F(WoCamera, origin), F(WoCamera, lower_left), F(WoCamera, horizontal), F(WoCamera, vertical),
    F(WoCamera, u), F(WoCamera, v), F(WoCamera, lens_radius), F(WoCamera, pad),
    T(WoFrame), F(WoFrame, width), F(WoFrame, height), F(WoFrame, spp), F(WoFrame, max_depth), F(WoFrame, seed),
    F(WoFrame, mode), F(WoFrame, sample_offset), F(WoFrame, tile_rows), F(WoFrame, rank), F(WoFrame, nranks),
    F(WoFrame, n_recs), F(WoFrame, n_prims), F(WoFrame, time_sec), F(WoFrame, sphere_y), F(WoFrame, inv_width),
    F(WoFrame, inv_height), F(WoFrame, cam), F(WoFrame, band_cycle), F(WoFrame, band_skip),
    T(Wo_Ray), F(Wo_Ray, origin), F(Wo_Ray, t_max), F(Wo_Ray, dir), F(Wo_Ray, reserved),
    T(Wo_RayHit), F(Wo_RayHit, t), F(Wo_RayHit, flags), F(Wo_RayHit, leaf), F(Wo_RayHit, node),
    F(Wo_RayHit, normal), F(Wo_RayHit, material),
    T(Wo_RayCrossing), F(Wo_RayCrossing, t), F(Wo_RayCrossing, flags), F(Wo_RayCrossing, leaf),
    F(Wo_RayCrossing, node),
    T(Wo_RaySpans), F(Wo_RaySpans, count), F(Wo_RaySpans, flags), F(Wo_RaySpans, length), F(Wo_RaySpans, stored),
    T(Wo_MassGrid), F(Wo_MassGrid, lo), F(Wo_MassGrid, hi), F(Wo_MassGrid, axis), F(Wo_MassGrid, nu), F(Wo_MassGrid, nv),
    F(Wo_MassGrid, v_begin), F(Wo_MassGrid, v_count), F(Wo_MassGrid, reserved),
    T(Wo_MassPlan), F(Wo_MassPlan, o_axis), F(Wo_MassPlan, pad), F(Wo_MassPlan, t_max), F(Wo_MassPlan, scale),
    F(Wo_MassPlan, k), F(Wo_MassPlan, q0), F(Wo_MassPlan, q1), F(Wo_MassPlan, u0), F(Wo_MassPlan, hu),
    F(Wo_MassPlan, v0), F(Wo_MassPlan, hv),
    T(Wo_MassSums), F(Wo_MassSums, lo), F(Wo_MassSums, hi), F(Wo_MassSums, rays), F(Wo_MassSums, rays_hit),
    F(Wo_MassSums, crossings), F(Wo_MassSums, reserved),
    T(Wo_MassProperties), F(Wo_MassProperties, volume), F(Wo_MassProperties, centroid), F(Wo_MassProperties, inertia),
    F(Wo_MassProperties, projected_area), F(Wo_MassProperties, cell), F(Wo_MassProperties, rays),
    F(Wo_MassProperties, crossings),
    T(Wo_FeatureIds), F(Wo_FeatureIds, node), F(Wo_FeatureIds, leaf), F(Wo_FeatureIds, material),
    F(Wo_FeatureIds, flags),
    T(Wo_DenoiseParams), F(Wo_DenoiseParams, levels), F(Wo_DenoiseParams, flags), F(Wo_DenoiseParams, k_color),
    F(Wo_DenoiseParams, k_normal), F(Wo_DenoiseParams, k_depth), F(Wo_DenoiseParams, reserved),
    T(Wo_MeshGrid), F(Wo_MeshGrid, lo), F(Wo_MeshGrid, hi), F(Wo_MeshGrid, n), F(Wo_MeshGrid, iters),
    F(Wo_MeshGrid, flags), F(Wo_MeshGrid, reserved),
    T(Wo_MeshVertex), F(Wo_MeshVertex, p), F(Wo_MeshVertex, cell),
    T(Wo_MeshQuad), F(Wo_MeshQuad, v),
    T(Wo_MeshQuadIds), F(Wo_MeshQuadIds, leaf), F(Wo_MeshQuadIds, node), F(Wo_MeshQuadIds, material),
    F(Wo_MeshQuadIds, flags),
    T(Wo_MeshCounts), F(Wo_MeshCounts, vertices), F(Wo_MeshCounts, quads), F(Wo_MeshCounts, cap_quads),
    F(Wo_MeshCounts, flags),
    T(Wo_Mesh), F(Wo_Mesh, vertices), F(Wo_Mesh, quads), F(Wo_Mesh, quad_ids), F(Wo_Mesh, counts),
};

#undef T
#undef F

size_t wo_abi_layout(char const* type, char const* field) {
    if (!type) return (size_t)-1;
    for (size_t i = 0; i < sizeof kAbi / sizeof kAbi[0]; ++i) {
        const AbiField* a = &kAbi[i];
        if (strcmp(a->type, type) != 0) continue;
        if (!field && !a->field) return a->value;
        if (field && a->field && strcmp(a->field, field) == 0) return a->value;
    }
    return (size_t)-1;
}
