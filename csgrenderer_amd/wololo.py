"""ctypes mirror of the wololo C API (libwololo.so).

The product is the C-ABI library built from ``csgrenderer_amd/csrc`` (HIP
kernels for gfx950 + C host).  This module only binds it -- same names and
argument meaning as the reference's ``src/wololo/renderer/renderer.h:18-33``
and ``src/wololo/app.h:20-30`` plus the extensions of
``include/wololo/renderer/renderer_ext.h`` -- so tests and ``bench.py`` read
like C callers.  There is no fallback: if the library is missing, loading
raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import (POINTER, Structure, c_bool, c_char_p, c_double, c_float, c_int, c_size_t, c_uint32,
                    c_ulonglong, c_void_p)

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# WOLOLO_LIB: another build of the same library (A/B measurements of build options)
LIB_PATH = os.environ.get("WOLOLO_LIB") or os.path.join(PKG_DIR, "lib", "libwololo.so")

# ---- wo_scene.h constants -------------------------------------------------------------------
WO_OP_PRIM, WO_OP_UNION, WO_OP_INTER, WO_OP_DIFF, WO_OP_RDIFF, WO_OP_BOUND = 1, 2, 3, 4, 5, 6
WO_LEAF_SPHERE, WO_LEAF_HALFSPACE = 16, 17
WO_MAT_LAMBERTIAN, WO_MAT_METAL, WO_MAT_DIELECTRIC = 0, 1, 2
MODE_UBERSHADER_RT1, MODE_DEBUG_ST, MODE_PATHTRACE, MODE_NORMALS = 0, 1, 2, 3
TRACER_AUTO, TRACER_INTERPRETER, TRACER_JIT, TRACER_LANES = 0, 1, 2, 3
TRACERS = {"auto": TRACER_AUTO, "interpreter": TRACER_INTERPRETER, "jit": TRACER_JIT, "lanes": TRACER_LANES}
WO_T_MIN = 1.0e-3
# wo_scene.h WO_WORK_* (executed-work counters)
WORK_KINDS = ("segments", "sphere_tests", "halfspace_tests", "bound_tests", "events", "sweep_steps", "recollects",
              "primary_segments", "cyc_take", "cyc_collect", "cyc_sweep", "cyc_shade", "cyc_loop", "idle_lanes",
              "sweep_trips", "cyc_cam")
WO_NODE_INVALID = 0xFFFFFFFF
# renderer_ext.h WO_RAY_* (Wo_RayHit.flags) and Wo_RayTracer
RAY_HIT, RAY_EXIT, RAY_ENTERS, RAY_INVALID = 1, 2, 4, 8
RAY_INSIDE, RAY_TRUNCATED = 16, 32  # Wo_RaySpans.flags
POINT_INSIDE, POINT_INVALID = 1, 8  # WO_POINT_*
RAY_TRACER_AUTO, RAY_TRACER_INTERPRETER, RAY_TRACER_LANES = 0, 1, 2
RAY_TRACERS = {"auto": RAY_TRACER_AUTO, "interpreter": RAY_TRACER_INTERPRETER, "lanes": RAY_TRACER_LANES}


class Vec3(Structure):
    _fields_ = [("x", c_double), ("y", c_double), ("z", c_double)]


class Quaternion(Structure):
    _fields_ = [("real", c_double), ("imaginary", Vec3)]


class NodeArgument(Structure):
    _fields_ = [("orientation", Quaternion), ("offset", Vec3), ("node", c_uint32)]


class RenderParams(Structure):
    _fields_ = [("width", c_uint32), ("height", c_uint32), ("spp", c_uint32), ("max_depth", c_uint32),
                ("seed", c_uint32), ("mode", c_uint32), ("sample_offset", c_uint32), ("time_sec", c_float)]


class WoRec(Structure):
    _fields_ = [("op", c_uint32), ("u0", c_uint32), ("u1", c_uint32), ("f", c_float * 5)]


class WoMaterial(Structure):
    _fields_ = [("kind", c_uint32), ("albedo", c_float * 3), ("fuzz", c_float), ("ior", c_float),
                ("inv_ior", c_float), ("r0", c_float)]


class WoCamera(Structure):
    _fields_ = [("origin", c_float * 3), ("lower_left", c_float * 3), ("horizontal", c_float * 3),
                ("vertical", c_float * 3), ("u", c_float * 3), ("v", c_float * 3), ("lens_radius", c_float),
                ("pad", c_float * 3)]


class WoFrame(Structure):
    _fields_ = [("width", c_uint32), ("height", c_uint32), ("spp", c_uint32), ("max_depth", c_uint32),
                ("seed", c_uint32), ("mode", c_uint32), ("sample_offset", c_uint32), ("tile_rows", c_uint32),
                ("rank", c_uint32), ("nranks", c_uint32), ("n_recs", c_uint32), ("n_prims", c_uint32),
                ("time_sec", c_float), ("sphere_y", c_float), ("inv_width", c_float), ("inv_height", c_float),
                ("cam", WoCamera), ("band_cycle", c_uint32), ("band_skip", c_uint32)]


class Ray(Structure):
    _fields_ = [("origin", c_float * 3), ("t_max", c_float), ("dir", c_float * 3), ("reserved", c_uint32)]


class RayHit(Structure):
    _fields_ = [("t", c_float), ("flags", c_uint32), ("leaf", c_uint32), ("node", c_uint32),
                ("normal", c_float * 3), ("material", c_uint32)]


# numpy view of a Wo_RayHit array (Renderer.trace_rays returns it)
RAY_HIT_FIELDS = [("t", "<f4"), ("flags", "<u4"), ("leaf", "<u4"), ("node", "<u4"), ("normal", "<f4", (3,)),
                  ("material", "<u4")]



class RayCrossing(Structure):
    _fields_ = [("t", c_float), ("flags", c_uint32), ("leaf", c_uint32), ("node", c_uint32)]


class RaySpans(Structure):
    _fields_ = [("count", c_uint32), ("flags", c_uint32), ("length", c_float), ("stored", c_uint32)]


# numpy views of Wo_RayCrossing / Wo_RaySpans arrays (Renderer.trace_spans returns them)
RAY_CROSSING_FIELDS = [("t", "<f4"), ("flags", "<u4"), ("leaf", "<u4"), ("node", "<u4")]
RAY_SPANS_FIELDS = [("count", "<u4"), ("flags", "<u4"), ("length", "<f4"), ("stored", "<u4")]


# renderer_ext.h Wo_MassGrid / Wo_MassPlan / Wo_MassSums / Wo_MassProperties (mass properties by ray-grid integration)
class MassGrid(Structure):
    _fields_ = [("lo", c_float * 3), ("hi", c_float * 3), ("axis", c_uint32), ("nu", c_uint32), ("nv", c_uint32),
                ("v_begin", c_uint32), ("v_count", c_uint32), ("reserved", c_uint32)]


class MassPlan(Structure):
    _fields_ = [("o_axis", c_float), ("pad", c_float), ("t_max", c_float), ("scale", c_float), ("k", ctypes.c_int32),
                ("q0", c_uint32), ("q1", c_uint32), ("u0", c_float), ("hu", c_float), ("v0", c_float), ("hv", c_float)]


class MassSums(Structure):
    _fields_ = [("lo", ctypes.c_uint64 * 10), ("hi", ctypes.c_uint64 * 10), ("rays", ctypes.c_uint64),
                ("rays_hit", ctypes.c_uint64), ("crossings", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]

    def as_dict(self):
        """{"sums": the ten sums as Python integers (lo + hi * 2^32), "lo", "hi", "rays", "rays_hit", "crossings"}."""
        lo, hi = [int(x) for x in self.lo], [int(x) for x in self.hi]
        return {"sums": [a + (b << 32) for a, b in zip(lo, hi)], "lo": lo, "hi": hi, "rays": int(self.rays),
                "rays_hit": int(self.rays_hit), "crossings": int(self.crossings)}


class MassProperties(Structure):
    _fields_ = [("volume", c_double), ("centroid", c_double * 3), ("inertia", c_double * 9),
                ("projected_area", c_double), ("cell", c_double * 3), ("rays", ctypes.c_uint64),
                ("crossings", ctypes.c_uint64)]


MASS_MAX_CELLS = 32768
assert ctypes.sizeof(MassGrid) == 48 and ctypes.sizeof(MassSums) == 192


# renderer_ext.h Wo_FeatureIds and the planes of wo_renderer_render_features[_device]
class FeatureIds(Structure):
    _fields_ = [("node", c_uint32), ("leaf", c_uint32), ("material", c_uint32), ("flags", c_uint32)]


# numpy view of the ids plane (Renderer.render_features returns it)
FEATURE_IDS_FIELDS = [("node", "<u4"), ("leaf", "<u4"), ("material", "<u4"), ("flags", "<u4")]
FEATURE_ALBEDO, FEATURE_NORMAL, FEATURE_IDS, FEATURE_PLANES = 0, 1, 2, 3
assert ctypes.sizeof(FeatureIds) == 16


# renderer_ext.h Wo_DenoiseParams (the a-trous denoiser guided by the feature planes)
class DenoiseParams(Structure):
    _fields_ = [("levels", c_uint32), ("flags", c_uint32), ("k_color", c_float), ("k_normal", c_float),
                ("k_depth", c_float), ("reserved", c_uint32)]


DENOISE_DEMODULATE, DENOISE_STOP_AT_NODES, DENOISE_MAX_LEVELS = 1, 2, 8
assert ctypes.sizeof(DenoiseParams) == 24


# renderer_ext.h Wo_MeshGrid ... Wo_Mesh (the closed quad mesh of the solid, surface nets on a uniform grid)
class MeshGrid(Structure):
    _fields_ = [("lo", c_float * 3), ("hi", c_float * 3), ("n", c_uint32 * 3), ("iters", c_uint32),
                ("flags", c_uint32), ("reserved", c_uint32)]


class MeshVertex(Structure):
    _fields_ = [("p", c_float * 3), ("cell", c_uint32)]


class MeshQuad(Structure):
    _fields_ = [("v", c_uint32 * 4)]


class MeshQuadIds(Structure):
    _fields_ = [("leaf", c_uint32), ("node", c_uint32), ("material", c_uint32), ("flags", c_uint32)]


class MeshCounts(Structure):
    _fields_ = [("vertices", c_uint32), ("quads", c_uint32), ("cap_quads", c_uint32), ("flags", c_uint32)]


class Mesh(Structure):
    _fields_ = [("vertices", POINTER(MeshVertex)), ("quads", POINTER(MeshQuad)), ("quad_ids", POINTER(MeshQuadIds)),
                ("counts", MeshCounts)]


# numpy views of Wo_MeshVertex / Wo_MeshQuadIds arrays (Renderer.mesh returns them; quads are (n, 4) uint32)
MESH_VERTEX_FIELDS = [("p", "<f4", (3,)), ("cell", "<u4")]
MESH_QUAD_IDS_FIELDS = [("leaf", "<u4"), ("node", "<u4"), ("material", "<u4"), ("flags", "<u4")]
MESH_MAX_CELLS, MESH_MAX_ITERS = 1024, 24
MESH_TRUNCATED = 1  # Wo_MeshCounts.flags
MESH_QUAD_AXIS, MESH_QUAD_POSITIVE, MESH_QUAD_CAP = 3, 4, 8  # Wo_MeshQuadIds.flags
assert ctypes.sizeof(MeshGrid) == 48 and ctypes.sizeof(MeshCounts) == 16
assert ctypes.sizeof(MeshVertex) == 16 and ctypes.sizeof(MeshQuad) == 16 and ctypes.sizeof(MeshQuadIds) == 16

assert ctypes.sizeof(Ray) == 32 and ctypes.sizeof(RayHit) == 32
assert ctypes.sizeof(RayCrossing) == 16 and ctypes.sizeof(RaySpans) == 16
assert ctypes.sizeof(Vec3) == 24 and ctypes.sizeof(Quaternion) == 32 and ctypes.sizeof(NodeArgument) == 64
assert ctypes.sizeof(WoRec) == 32 and ctypes.sizeof(WoMaterial) == 32

# Every exported symbol and its signature (restype, argtypes).  tests/ check that the
# library exports exactly these names (the C-ABI declared in include/wololo/*.h).
_R = POINTER(ctypes.c_char)  # opaque Wo_Renderer*
SIGNATURES = {
    # renderer.h (reference API)
    "wo_renderer_new": (c_void_p, [c_void_p, c_char_p, c_size_t]),
    "wo_renderer_del": (None, [c_void_p]),
    "wo_renderer_draw_frame": (None, [c_void_p]),
    "wo_renderer_add_sphere_node": (c_uint32, [c_void_p, c_double]),
    "wo_renderer_add_infinite_planar_partition_node": (c_uint32, [c_void_p, Vec3]),
    "wo_renderer_add_union_of_node": (c_uint32, [c_void_p, NodeArgument, NodeArgument]),
    "wo_renderer_add_intersection_of_node": (c_uint32, [c_void_p, NodeArgument, NodeArgument]),
    "wo_renderer_add_difference_of_node": (c_uint32, [c_void_p, NodeArgument, NodeArgument]),
    "wo_renderer_isroot": (c_bool, [c_void_p, c_uint32]),
    # app.h (reference API + extensions)
    "wo_app_new": (c_void_p, [c_double, c_uint32, c_uint32, c_char_p, c_void_p, c_void_p, c_void_p]),
    "wo_app_run": (c_bool, [c_void_p]),
    "wo_app_swap_scene": (None, [c_void_p, c_void_p]),
    "wo_app_glfw_window": (c_void_p, [c_void_p]),
    "wo_app_window_width": (c_uint32, [c_void_p]),
    "wo_app_window_height": (c_uint32, [c_void_p]),
    "wo_app_time_sec": (c_double, [c_void_p]),
    # renderer_ext.h
    "wo_render_params_default": (None, [POINTER(RenderParams)]),
    "wo_renderer_add_lambertian_material": (c_uint32, [c_void_p, Vec3]),
    "wo_renderer_add_metal_material": (c_uint32, [c_void_p, Vec3, c_double]),
    "wo_renderer_add_dielectric_material": (c_uint32, [c_void_p, c_double]),
    "wo_renderer_set_node_material": (c_bool, [c_void_p, c_uint32, c_uint32]),
    "wo_renderer_set_camera": (None, [c_void_p, Vec3, Vec3, Vec3, c_double, c_double, c_double]),
    "wo_renderer_set_draw_params": (None, [c_void_p, POINTER(RenderParams), c_int]),
    "wo_renderer_render_f32": (c_int, [c_void_p, POINTER(RenderParams), c_void_p]),
    "wo_renderer_render_rows_device": (c_int, [c_void_p, POINTER(RenderParams), c_void_p, c_uint32, c_uint32,
                                               c_uint32, c_void_p, c_void_p]),
    "wo_renderer_count_work": (c_int, [c_void_p, POINTER(RenderParams), c_uint32, c_uint32, c_uint32,
                                       POINTER(c_ulonglong)]),
    "wo_assemble_rows_device": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_uint32, c_void_p]),
    "wo_assemble_rows_device_ex": (c_int, [c_void_p, c_void_p, c_uint32, c_uint32, c_uint32, c_uint32, c_uint32,
                                           c_uint32, c_void_p]),
    "wo_renderer_set_band_weight": (c_int, [c_void_p, c_uint32, c_uint32]),
    "wo_renderer_set_devices": (c_int, [c_void_p, c_int]),
    "wo_renderer_device_count": (c_int, [c_void_p]),
    "wo_renderer_frame_ranks": (c_int, [c_void_p, POINTER(RenderParams)]),
    "wo_renderer_peer_mode": (c_int, [c_void_p, c_int]),
    "wo_renderer_render_frame_device": (c_int, [c_void_p, POINTER(RenderParams), c_void_p, c_void_p]),
    "wo_renderer_take_segments": (c_int, [c_void_p, POINTER(c_ulonglong)]),
    "wo_renderer_finish": (c_int, [c_void_p]),
    "wo_renderer_last_frame": (POINTER(c_float), [c_void_p, POINTER(c_uint32), POINTER(c_uint32)]),
    "wo_renderer_last_frame_bgra8": (POINTER(c_uint32), [c_void_p, POINTER(c_uint32), POINTER(c_uint32)]),
    "wo_renderer_set_map_float": (None, [c_void_p, c_int]),
    "wo_renderer_set_frame_stamps": (c_int, [c_void_p, c_int]),
    "wo_renderer_frame_stamps": (c_int, [c_void_p, POINTER(c_double), c_int]),
    "wo_srgb8_thresholds": (None, [POINTER(c_float)]),
    "wo_srgb8_encode_device": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "wo_srgb8_encode_host": (None, [c_void_p, c_void_p, c_size_t]),
    "wo_renderer_set_progressive": (None, [c_void_p, c_int]),
    "wo_renderer_accumulated_spp": (c_uint32, [c_void_p]),
    "wo_renderer_render_accumulate": (c_int, [c_void_p, POINTER(RenderParams), c_void_p, c_int]),
    "wo_renderer_compile": (c_int, [c_void_p]),
    "wo_renderer_program": (POINTER(WoRec), [c_void_p, POINTER(c_uint32), POINTER(c_uint32)]),
    "wo_renderer_materials": (POINTER(WoMaterial), [c_void_p, POINTER(c_uint32)]),
    "wo_renderer_frame_desc": (c_int, [c_void_p, POINTER(RenderParams), c_uint32, c_uint32, c_uint32,
                                       POINTER(WoFrame)]),
    "wo_renderer_set_jit": (None, [c_void_p, c_int]),
    "wo_renderer_set_tracer": (None, [c_void_p, c_int]),
    "wo_renderer_trace_path": (c_char_p, [c_void_p]),
    "wo_renderer_trace_rays_device": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wo_renderer_trace_rays": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "wo_renderer_pixel_ray": (c_int, [c_void_p, POINTER(RenderParams), c_uint32, c_uint32, POINTER(Ray)]),
    "wo_renderer_pick": (c_int, [c_void_p, POINTER(RenderParams), c_uint32, c_uint32, POINTER(RayHit)]),
    "wo_renderer_program_nodes": (POINTER(c_uint32), [c_void_p, POINTER(c_uint32)]),
    "wo_renderer_set_ray_tracer": (None, [c_void_p, c_int]),
    "wo_renderer_ray_path": (c_char_p, [c_void_p]),
    "wo_renderer_trace_spans_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_uint32, c_void_p]),
    "wo_renderer_trace_spans": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_uint32]),
    "wo_renderer_classify_points_device": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "wo_renderer_classify_points": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "wo_mass_grid_plan": (c_int, [POINTER(MassGrid), POINTER(MassPlan)]),
    "wo_mass_properties_from_sums": (c_int, [POINTER(MassGrid), POINTER(MassSums), POINTER(MassProperties)]),
    "wo_renderer_mass_sums_device": (c_int, [c_void_p, POINTER(MassGrid), c_void_p, c_void_p]),
    "wo_renderer_mass_properties": (c_int, [c_void_p, POINTER(MassGrid), POINTER(MassProperties), POINTER(MassSums)]),
    "wo_renderer_render_features_device": (c_int, [c_void_p, POINTER(RenderParams), c_void_p, c_size_t, c_uint32,
                                                   c_uint32, c_uint32, c_void_p]),
    "wo_renderer_render_features": (c_int, [c_void_p, POINTER(RenderParams), c_void_p]),
    "wo_denoise_params_default": (None, [POINTER(DenoiseParams)]),
    "wo_denoise_scratch_bytes": (c_size_t, [c_uint32, c_uint32, POINTER(DenoiseParams)]),
    "wo_denoise_device": (c_int, [POINTER(DenoiseParams), c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_size_t, c_void_p]),
    "wo_denoise_host": (c_int, [POINTER(DenoiseParams), c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "wo_renderer_render_denoised": (c_int, [c_void_p, POINTER(RenderParams), POINTER(DenoiseParams), c_void_p]),
    "wo_mesh_grid_check": (c_int, [POINTER(MeshGrid), POINTER(c_float)]),
    "wo_mesh_scratch_bytes": (c_size_t, [POINTER(MeshGrid)]),
    "wo_renderer_mesh_device": (c_int, [c_void_p, POINTER(MeshGrid), c_void_p, c_uint32, c_void_p, c_void_p, c_uint32,
                                        c_void_p, c_void_p, c_size_t, c_void_p]),
    "wo_renderer_mesh": (c_int, [c_void_p, POINTER(MeshGrid), POINTER(Mesh)]),
    "wo_mesh_free": (None, [POINTER(Mesh)]),
    "wo_mesh_write_obj": (c_int, [c_char_p, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32]),
    "wo_renderer_set_jit_async": (None, [c_void_p, c_int]),
    "wo_renderer_jit_pending": (c_int, [c_void_p]),
    "wo_renderer_prepare": (c_int, [c_void_p]),
    "wo_renderer_jit_source": (c_void_p, [c_void_p]),
    "wo_jit_compile_check": (c_int, [c_char_p, c_char_p, c_char_p, c_size_t]),
    "wo_jit_code_resources": (c_int, [c_char_p, c_char_p, POINTER(ctypes.c_uint32), c_char_p, ctypes.c_size_t]),
    "wo_jit_code_object": (ctypes.c_longlong, [c_char_p, c_char_p, POINTER(c_int), POINTER(c_double), c_char_p,
                                               c_char_p, c_size_t]),
    "wo_renderer_jit_info": (c_int, [c_void_p, POINTER(c_double)]),
    "wo_renderer_lanes_info": (c_int, [c_void_p, POINTER(c_uint32)]),
    "wo_renderer_kernel_info": (c_int, [c_void_p, c_char_p, POINTER(c_uint32)]),
    "wo_free": (None, [c_void_p]),
    "wo_renderer_node_count": (c_size_t, [c_void_p]),
    "wo_renderer_name": (c_char_p, [c_void_p]),
    "wo_renderer_device": (c_int, [c_void_p]),
    "wo_renderer_last_error": (c_char_p, []),
    "wo_renderer_clear_error": (None, []),
    "wo_version": (c_char_p, []),
    "wo_abi_layout": (c_size_t, [c_char_p, c_char_p]),
    "wo_hip_device_count": (c_int, []),
    "wo_hip_runtime_version": (c_int, []),
    "wo_fastmath_check": (c_int, [c_int, c_uint32, c_uint32, POINTER(c_ulonglong), POINTER(c_uint32)]),
}

_lib = None


def load(path: str | None = None) -> ctypes.CDLL:
    """Load libwololo.so (raises if it has not been built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(f"libwololo.so not found at {p}; build it with `python -c 'import __graft_entry__ as g; "
                           f"g.build()'` or `make -C csgrenderer_amd/csrc`")
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        if os.environ.get("WOLOLO_LIB") and not hasattr(lib, name):
            continue  # an older build under A/B measurement: bind what it has
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def vec3(x, y, z) -> Vec3:
    return Vec3(float(x), float(y), float(z))


def quat_identity() -> Quaternion:
    return Quaternion(1.0, Vec3(0.0, 0.0, 0.0))


def arg(node: int, offset=(0.0, 0.0, 0.0), orientation: Quaternion | None = None) -> NodeArgument:
    return NodeArgument(orientation or quat_identity(), vec3(*offset), int(node))


def last_error() -> str:
    e = load().wo_renderer_last_error()
    return e.decode() if e else ""


def clear_error():
    load().wo_renderer_clear_error()


class WololoError(RuntimeError):
    pass


class Renderer:
    """Thin owner of a Wo_Renderer* (all calls go straight to the C library)."""

    def __init__(self, name: str = "py", max_nodes: int = 1024, app: int | None = None):
        self.lib = load()
        self.ptr = self.lib.wo_renderer_new(app, name.encode(), max_nodes)
        if not self.ptr:
            raise WololoError(f"wo_renderer_new failed: {last_error()}")

    def close(self):
        if self.ptr:
            self.lib.wo_renderer_del(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- nodes (reference API) ----
    def _check(self, n: int) -> int:
        if n == WO_NODE_INVALID:
            raise WololoError(last_error())
        return n

    def sphere(self, radius: float) -> int:
        return self._check(self.lib.wo_renderer_add_sphere_node(self.ptr, float(radius)))

    def halfspace(self, normal) -> int:
        return self._check(self.lib.wo_renderer_add_infinite_planar_partition_node(self.ptr, vec3(*normal)))

    def union(self, a: NodeArgument, b: NodeArgument) -> int:
        return self._check(self.lib.wo_renderer_add_union_of_node(self.ptr, a, b))

    def intersection(self, a: NodeArgument, b: NodeArgument) -> int:
        return self._check(self.lib.wo_renderer_add_intersection_of_node(self.ptr, a, b))

    def difference(self, a: NodeArgument, b: NodeArgument) -> int:
        return self._check(self.lib.wo_renderer_add_difference_of_node(self.ptr, a, b))

    def isroot(self, n: int) -> bool:
        return bool(self.lib.wo_renderer_isroot(self.ptr, n))

    # ---- extensions ----
    def lambertian(self, albedo) -> int:
        return self.lib.wo_renderer_add_lambertian_material(self.ptr, vec3(*albedo))

    def metal(self, albedo, fuzz: float) -> int:
        return self.lib.wo_renderer_add_metal_material(self.ptr, vec3(*albedo), float(fuzz))

    def dielectric(self, ior: float) -> int:
        return self.lib.wo_renderer_add_dielectric_material(self.ptr, float(ior))

    def set_material(self, leaf: int, mat: int):
        if not self.lib.wo_renderer_set_node_material(self.ptr, leaf, mat):
            raise WololoError(f"set_node_material({leaf}, {mat}) rejected")

    def set_camera(self, look_from, look_at, vup=(0, 1, 0), vfov=90.0, aperture=0.0, focus_dist=1.0):
        self.lib.wo_renderer_set_camera(self.ptr, vec3(*look_from), vec3(*look_at), vec3(*vup), float(vfov),
                                        float(aperture), float(focus_dist))

    def compile(self) -> int:
        n = self.lib.wo_renderer_compile(self.ptr)
        if n < 0:
            raise WololoError(last_error())
        return n

    def program(self):
        """(records ctypes array, n_prims) of the compiled scene."""
        nr, npr = c_uint32(0), c_uint32(0)
        p = self.lib.wo_renderer_program(self.ptr, ctypes.byref(nr), ctypes.byref(npr))
        if not p:
            raise WololoError(last_error())
        arr = (WoRec * max(nr.value, 1))()
        if nr.value:
            ctypes.memmove(arr, p, ctypes.sizeof(WoRec) * nr.value)
        return arr, nr.value, npr.value

    def materials(self):
        n = c_uint32(0)
        p = self.lib.wo_renderer_materials(self.ptr, ctypes.byref(n))
        arr = (WoMaterial * max(n.value, 1))()
        ctypes.memmove(arr, p, ctypes.sizeof(WoMaterial) * n.value)
        return arr, n.value

    def jit_source(self) -> str | None:
        p = self.lib.wo_renderer_jit_source(self.ptr)
        if not p:
            return None
        try:
            return ctypes.string_at(p).decode()
        finally:
            self.lib.wo_free(p)

    def jit_info(self):
        """(origin, seconds) of the specialised kernel: origin "process" / "disk" / "compiled", or None."""
        sec = c_double(0.0)
        o = self.lib.wo_renderer_jit_info(self.ptr, ctypes.byref(sec))
        return (None if o < 0 else JIT_ORIGINS[o]), sec.value

    def lanes_info(self):
        """The lane tracer's BVH: {"nodes", "depth", "top", "always", "kind"} ("kind": the kernel
        form of the last path or ray launch, wo_dev_impl.h PathKind), or None if not on the lane tracer."""
        out = (c_uint32 * 5)()
        if self.lib.wo_renderer_lanes_info(self.ptr, out) < 0:
            return None
        return dict(zip(("nodes", "depth", "top", "always", "kind"), list(out)))

    def set_jit(self, mode: int):
        self.lib.wo_renderer_set_jit(self.ptr, int(mode))

    def set_tracer(self, tracer):
        """TRACER_AUTO / _INTERPRETER / _JIT / _LANES, or the names "auto", "interpreter", "jit", "lanes"."""
        if isinstance(tracer, str):
            tracer = TRACERS[tracer]
        self.lib.wo_renderer_set_tracer(self.ptr, int(tracer))

    def set_jit_async(self, on: bool):
        self.lib.wo_renderer_set_jit_async(self.ptr, 1 if on else 0)

    def jit_pending(self) -> bool:
        return bool(self.lib.wo_renderer_jit_pending(self.ptr))

    def kernel_info(self):
        """The last launch's path kernel as loaded (renderer_ext.h wo_renderer_kernel_info):
        {"key", "kind", "scratch_bytes", "vgprs", "lds_bytes"}, or None before a path launch."""
        key = ctypes.create_string_buffer(65)
        out = (c_uint32 * 4)()
        if self.lib.wo_renderer_kernel_info(self.ptr, key, out) != 0:
            return None
        return {"key": key.value.decode(), "kind": int(out[0]), "scratch_bytes": int(out[1]),
                "vgprs": int(out[2]), "lds_bytes": int(out[3])}

    def prepare(self):
        """Compile, upload and load the scene's kernels now, waiting for a background
        compile (renderer_ext.h wo_renderer_prepare)."""
        if self.lib.wo_renderer_prepare(self.ptr) != 0:
            raise WololoError(last_error())

    def trace_path(self) -> str:
        return self.lib.wo_renderer_trace_path(self.ptr).decode()

    # ---- ray queries (renderer_ext.h wo_renderer_trace_rays ...) ----
    def trace_rays(self, rays):
        """Trace n rays given as an (n, 8) float32 array of Wo_Ray rows (origin, t_max, dir,
        reserved); returns a structured array of n Wo_RayHit (RAY_HIT_FIELDS).  Synchronous."""
        import numpy as np
        a = np.ascontiguousarray(rays, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != 8:
            raise ValueError("rays: an (n, 8) float32 array")
        out = np.zeros(a.shape[0], dtype=np.dtype(RAY_HIT_FIELDS))
        if self.lib.wo_renderer_trace_rays(self.ptr, a.ctypes.data_as(c_void_p), out.ctypes.data_as(c_void_p),
                                           a.shape[0]):
            raise WololoError(last_error())
        return out

    def trace_rays_device(self, d_rays: int, d_hits: int, n: int, stream: int = 0):
        """n Wo_Ray at device address d_rays -> n Wo_RayHit at d_hits, asynchronously on `stream`."""
        if self.lib.wo_renderer_trace_rays_device(self.ptr, c_void_p(d_rays or None), c_void_p(d_hits or None),
                                                  int(n), c_void_p(stream or None)):
            raise WololoError(last_error())

    def pixel_ray(self, params: RenderParams, x: int, y: int):
        """The pixel-centre ray of a NORMALS frame as a Wo_Ray row: (8,) float32."""
        import numpy as np
        ray = Ray()
        if self.lib.wo_renderer_pixel_ray(self.ptr, ctypes.byref(params), int(x), int(y), ctypes.byref(ray)):
            raise WololoError(last_error())
        return np.frombuffer(bytes(ray), dtype=np.float32).copy()

    def pick(self, params: RenderParams, x: int, y: int):
        """The Wo_RayHit under pixel (x, y): a structured scalar (RAY_HIT_FIELDS)."""
        import numpy as np
        hit = RayHit()
        if self.lib.wo_renderer_pick(self.ptr, ctypes.byref(params), int(x), int(y), ctypes.byref(hit)):
            raise WololoError(last_error())
        return np.frombuffer(bytes(hit), dtype=np.dtype(RAY_HIT_FIELDS))[0]

    def program_nodes(self):
        """Per compiled record its source node handle (WO_NODE_INVALID for non-leaf records)."""
        import numpy as np
        n = c_uint32(0)
        p = self.lib.wo_renderer_program_nodes(self.ptr, ctypes.byref(n))
        if not p:
            raise WololoError(last_error())
        if not n.value:
            return np.zeros(0, dtype=np.uint32)
        return np.ctypeslib.as_array(p, shape=(n.value,)).astype(np.uint32)

    def set_ray_tracer(self, tracer):
        """RAY_TRACER_AUTO / _INTERPRETER / _LANES, or the names "auto", "interpreter", "lanes"."""
        if isinstance(tracer, str):
            tracer = RAY_TRACERS[tracer]
        self.lib.wo_renderer_set_ray_tracer(self.ptr, int(tracer))

    def ray_path(self) -> str:
        return self.lib.wo_renderer_ray_path(self.ptr).decode()

    # ---- ray span queries and point classification (renderer_ext.h wo_renderer_trace_spans ...) ----
    def trace_spans(self, rays, max_crossings: int, crossings=None):
        """Every crossing of n rays ((n, 8) float32 Wo_Ray rows) with the solid: returns
        (spans[n], crossings[max_crossings, n]) as structured arrays (RAY_SPANS_FIELDS,
        RAY_CROSSING_FIELDS); row k of `crossings` holds every ray's k-th crossing, valid for
        k < spans["stored"].  `crossings`: a (max_crossings, n) array to fill instead of a new
        zeroed one (rows that are not written keep its content).  Synchronous."""
        import numpy as np
        a = np.ascontiguousarray(rays, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != 8:
            raise ValueError("rays: an (n, 8) float32 array")
        n, m = a.shape[0], int(max_crossings)
        spans = np.zeros(n, dtype=np.dtype(RAY_SPANS_FIELDS))
        if crossings is None:
            crossings = np.zeros((m, n), dtype=np.dtype(RAY_CROSSING_FIELDS))
        elif (crossings.dtype != np.dtype(RAY_CROSSING_FIELDS) or crossings.shape != (m, n)
              or not crossings.flags.c_contiguous or not crossings.flags.writeable):
            raise ValueError("crossings: a writable C-contiguous (max_crossings, n) RAY_CROSSING_FIELDS array")
        if self.lib.wo_renderer_trace_spans(self.ptr, a.ctypes.data_as(c_void_p), spans.ctypes.data_as(c_void_p),
                                            crossings.ctypes.data_as(c_void_p) if m else None, n, m):
            raise WololoError(last_error())
        return spans, crossings

    def trace_spans_device(self, d_rays: int, d_spans: int, d_crossings: int, n: int, max_crossings: int,
                           stream: int = 0):
        """n Wo_Ray at device address d_rays -> n Wo_RaySpans at d_spans and the crossing-major
        Wo_RayCrossing rows at d_crossings (0 with max_crossings = 0), asynchronously on `stream`."""
        if self.lib.wo_renderer_trace_spans_device(self.ptr, c_void_p(d_rays or None), c_void_p(d_spans or None),
                                                   c_void_p(d_crossings or None), int(n), int(max_crossings),
                                                   c_void_p(stream or None)):
            raise WololoError(last_error())

    def classify_points(self, points):
        """WO_POINT_INSIDE / 0 / WO_POINT_INVALID per point of an (n, 3) or (n, 4) float32 array
        (a fourth column is ignored): uint32[n].  Synchronous."""
        import numpy as np
        p = np.asarray(points, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] not in (3, 4):
            raise ValueError("points: an (n, 3) or (n, 4) float32 array")
        a = np.zeros((p.shape[0], 4), dtype=np.float32)
        a[:, :p.shape[1]] = p
        out = np.zeros(p.shape[0], dtype=np.uint32)
        if self.lib.wo_renderer_classify_points(self.ptr, a.ctypes.data_as(c_void_p), out.ctypes.data_as(c_void_p),
                                                p.shape[0]):
            raise WololoError(last_error())
        return out

    def classify_points_device(self, d_points: int, d_out: int, n: int, stream: int = 0):
        """n float4 points at device address d_points -> n uint32 at d_out, asynchronously on `stream`."""
        if self.lib.wo_renderer_classify_points_device(self.ptr, c_void_p(d_points or None), c_void_p(d_out or None),
                                                       int(n), c_void_p(stream or None)):
            raise WololoError(last_error())

    # ---- mass properties (renderer_ext.h wo_renderer_mass_sums_device ...) ----
    def mass_sums_device(self, grid: MassGrid, d_sums: int, stream: int = 0):
        """Adds the exact sums of the grid's row range into the Wo_MassSums (192 bytes, zeroed by
        the caller) at device address d_sums, asynchronously on `stream`."""
        if self.lib.wo_renderer_mass_sums_device(self.ptr, ctypes.byref(grid), c_void_p(d_sums or None),
                                                 c_void_p(stream or None)):
            raise WololoError(last_error())

    def mass_properties(self, grid: MassGrid):
        """(MassProperties, MassSums) of the solid inside the grid's clip box.  Synchronous."""
        props, sums = MassProperties(), MassSums()
        if self.lib.wo_renderer_mass_properties(self.ptr, ctypes.byref(grid), ctypes.byref(props), ctypes.byref(sums)):
            raise WololoError(last_error())
        return props, sums

    # ---- surface mesh of the solid (renderer_ext.h wo_renderer_mesh ...) ----
    def mesh(self, grid: MeshGrid):
        """The closed quad mesh of the solid clipped to the grid's box: (vertices[V] of
        MESH_VERTEX_FIELDS, quads (Q, 4) uint32, ids[Q] of MESH_QUAD_IDS_FIELDS, MeshCounts).
        Synchronous; the arrays are copies, the library's own are released."""
        import numpy as np
        m = Mesh()
        if self.lib.wo_renderer_mesh(self.ptr, ctypes.byref(grid) if grid is not None else None, ctypes.byref(m)):
            raise WololoError(last_error())
        try:
            nv, nq = int(m.counts.vertices), int(m.counts.quads)
            vertices = np.zeros(nv, dtype=np.dtype(MESH_VERTEX_FIELDS))
            quads = np.zeros((nq, 4), dtype=np.uint32)
            ids = np.zeros(nq, dtype=np.dtype(MESH_QUAD_IDS_FIELDS))
            if nv:
                ctypes.memmove(vertices.ctypes.data, m.vertices, 16 * nv)
            if nq:
                ctypes.memmove(quads.ctypes.data, m.quads, 16 * nq)
                ctypes.memmove(ids.ctypes.data, m.quad_ids, 16 * nq)
            counts = MeshCounts(m.counts.vertices, m.counts.quads, m.counts.cap_quads, m.counts.flags)
        finally:
            self.lib.wo_mesh_free(ctypes.byref(m))
        return vertices, quads, ids, counts

    def mesh_device(self, grid: MeshGrid, d_vertices: int, max_vertices: int, d_quads: int, d_quad_ids: int,
                    max_quads: int, d_counts: int, d_scratch: int, scratch_bytes: int, stream: int = 0):
        """The mesh into device memory (16-byte rows at d_vertices, d_quads and, unless 0, d_quad_ids;
        the Wo_MeshCounts at d_counts), asynchronously on `stream`; d_scratch holds at least
        mesh_scratch_bytes(grid) bytes.  With both maxima 0 only the counts are made."""
        if self.lib.wo_renderer_mesh_device(self.ptr, ctypes.byref(grid) if grid is not None else None,
                                            c_void_p(d_vertices or None), int(max_vertices), c_void_p(d_quads or None),
                                            c_void_p(d_quad_ids or None), int(max_quads), c_void_p(d_counts or None),
                                            c_void_p(d_scratch or None), int(scratch_bytes), c_void_p(stream or None)):
            raise WololoError(last_error())

    # ---- first-hit feature buffers (renderer_ext.h wo_renderer_render_features ...) ----
    def render_features(self, params: RenderParams):
        """The feature planes of a PATHTRACE frame: (albedo (H, W, 4) float32 with w = coverage,
        normal (H, W, 4) float32 with w = mean hit depth, ids (H, W) FEATURE_IDS_FIELDS).  Synchronous."""
        import numpy as np
        h, w = int(params.height), int(params.width)
        out = np.zeros((FEATURE_PLANES, h, w, 4), dtype=np.float32)
        if self.lib.wo_renderer_render_features(self.ptr, ctypes.byref(params), out.ctypes.data_as(c_void_p)):
            raise WololoError(last_error())
        ids = out[FEATURE_IDS].view(np.uint32).reshape(h, w, 4).view(np.dtype(FEATURE_IDS_FIELDS)).reshape(h, w)
        return out[FEATURE_ALBEDO], out[FEATURE_NORMAL], ids

    def render_features_device(self, params: RenderParams, d_out: int, plane_stride: int, tile_rows: int, rank: int,
                               nranks: int, stream: int = 0):
        """This rank's rows of the three planes into device memory at d_out (plane p of local pixel i
        is the 16-byte row p * plane_stride + i), asynchronously on `stream`."""
        if self.lib.wo_renderer_render_features_device(self.ptr, ctypes.byref(params) if params is not None else None,
                                                       c_void_p(d_out or None), int(plane_stride), tile_rows, rank,
                                                       nranks, c_void_p(stream or None)):
            raise WololoError(last_error())

    def render_denoised(self, params: RenderParams, dp: "DenoiseParams | None" = None):
        """The denoised PATHTRACE frame of `params` ((H, W, 4) float32): the frame, its feature planes
        and wo_denoise_device on the renderer's device, then one copy.  dp None = the defaults."""
        import numpy as np
        out = np.zeros((int(params.height), int(params.width), 4), dtype=np.float32)
        if self.lib.wo_renderer_render_denoised(self.ptr, ctypes.byref(params), ctypes.byref(dp) if dp is not None else None,
                                                out.ctypes.data_as(c_void_p)):
            raise WololoError(last_error())
        return out

    def frame_desc(self, params: RenderParams, tile_rows=16, rank=0, nranks=1) -> WoFrame:
        fr = WoFrame()
        if self.lib.wo_renderer_frame_desc(self.ptr, ctypes.byref(params), tile_rows, rank, nranks,
                                           ctypes.byref(fr)):
            raise WololoError(last_error())
        return fr

    def render(self, params: RenderParams):
        """Full frame to host; returns a float32 numpy array (H, W, 4)."""
        import numpy as np
        out = np.empty((params.height, params.width, 4), dtype=np.float32)
        if self.lib.wo_renderer_render_f32(self.ptr, ctypes.byref(params), out.ctypes.data_as(c_void_p)):
            raise WololoError(last_error())
        return out

    def render_accumulate(self, params: RenderParams, reset: bool = False):
        """params.spp more samples into the progressive accumulation; returns (mean image, total spp)."""
        import numpy as np
        out = np.empty((params.height, params.width, 4), dtype=np.float32)
        n = self.lib.wo_renderer_render_accumulate(self.ptr, ctypes.byref(params), out.ctypes.data_as(c_void_p),
                                                   1 if reset else 0)
        if n < 0:
            raise WololoError(last_error())
        return out, n

    def draw_frame(self):
        """wo_renderer_draw_frame (pipelined: presents the previous frame)."""
        self.lib.wo_renderer_draw_frame(self.ptr)

    def set_devices(self, n: int) -> int:
        """Split every frame over n ranks (renderer_ext.h wo_renderer_set_devices)."""
        rc = self.lib.wo_renderer_set_devices(self.ptr, int(n))
        if rc < 0:
            raise WololoError(last_error())
        return rc

    def device_count(self) -> int:
        return int(self.lib.wo_renderer_device_count(self.ptr))

    def frame_ranks(self, params: RenderParams) -> int:
        """Ranks a frame with these parameters is split over (wo_renderer_frame_ranks)."""
        return int(self.lib.wo_renderer_frame_ranks(self.ptr, ctypes.byref(params)))

    def peer_mode(self, rank: int) -> str | None:
        """How rank `rank`'s share reaches rank 0: "same", "dma" or "staged" (None for rank 0)."""
        m = self.lib.wo_renderer_peer_mode(self.ptr, int(rank))
        return None if m < 0 else PEER_MODES[m]

    def render_frame_device(self, params: RenderParams, d_frame: int, stream: int = 0):
        """Whole frame over the renderer's ranks into device memory (wo_renderer_render_frame_device)."""
        if self.lib.wo_renderer_render_frame_device(self.ptr, ctypes.byref(params), c_void_p(d_frame),
                                                    c_void_p(stream or None)):
            raise WololoError(last_error())

    def take_segments(self) -> int:
        """Segments traced by render_frame_device frames since the last call (all ranks)."""
        t = c_ulonglong(0)
        if self.lib.wo_renderer_take_segments(self.ptr, ctypes.byref(t)):
            raise WololoError(last_error())
        return int(t.value)

    def finish(self):
        if self.lib.wo_renderer_finish(self.ptr):
            raise WololoError(last_error())

    def last_frame(self):
        """Copy of the last presented frame (H, W, 4) or None."""
        import numpy as np
        w, h = c_uint32(0), c_uint32(0)
        p = self.lib.wo_renderer_last_frame(self.ptr, ctypes.byref(w), ctypes.byref(h))
        if not p:
            return None
        return np.ctypeslib.as_array(p, shape=(h.value * w.value * 4,)).reshape(h.value, w.value, 4).copy()

    def last_frame_bgra8(self):
        """Copy of the last presented frame's present encode, (H, W) uint32 B8G8R8A8 sRGB, or None."""
        import numpy as np
        w, h = c_uint32(0), c_uint32(0)
        p = self.lib.wo_renderer_last_frame_bgra8(self.ptr, ctypes.byref(w), ctypes.byref(h))
        if not p:
            return None
        return np.ctypeslib.as_array(p, shape=(h.value * w.value,)).reshape(h.value, w.value).copy()

    def set_map_float(self, every_frame: bool):
        """Map every presented frame's float pixels back (True) or only when last_frame() asks (default)."""
        self.lib.wo_renderer_set_map_float(self.ptr, 1 if every_frame else 0)

    def set_frame_stamps(self, on: bool):
        if self.lib.wo_renderer_set_frame_stamps(self.ptr, 1 if on else 0):
            raise WololoError(last_error())

    def frame_stamps(self):
        """Logged pipeline stamps, a list of (render_begin, render_end, mapback_end) ms per presented frame."""
        buf = (c_double * (3 * 256))()
        n = self.lib.wo_renderer_frame_stamps(self.ptr, buf, 256)
        if n < 0:
            raise WololoError(last_error())
        return [tuple(buf[3 * i:3 * i + 3]) for i in range(n)]

    def set_draw_params(self, params: RenderParams, pin_time: bool = True):
        self.lib.wo_renderer_set_draw_params(self.ptr, ctypes.byref(params), 1 if pin_time else 0)

    def set_progressive(self, on: bool):
        self.lib.wo_renderer_set_progressive(self.ptr, 1 if on else 0)

    def accumulated_spp(self) -> int:
        return int(self.lib.wo_renderer_accumulated_spp(self.ptr))

    def count_work(self, params: RenderParams, tile_rows: int = 4, rank: int = 0, nranks: int = 1) -> dict:
        """Executed-work counters of one frame (wo_renderer_count_work), by WORK_KINDS name."""
        c = (c_ulonglong * len(WORK_KINDS))()
        if self.lib.wo_renderer_count_work(self.ptr, ctypes.byref(params), tile_rows, rank, nranks, c):
            raise WololoError(last_error())
        return dict(zip(WORK_KINDS, (int(v) for v in c)))

    def set_band_weight(self, cycle: int, skip: int):
        """Weighted row bands of multi-rank frames: rank 0 sits out `skip` of every `cycle` rounds."""
        if self.lib.wo_renderer_set_band_weight(self.ptr, cycle, skip):
            raise WololoError(last_error())

    def render_rows_device(self, params: RenderParams, d_out: int, tile_rows: int, rank: int, nranks: int,
                           stream: int = 0, d_segments: int = 0):
        if self.lib.wo_renderer_render_rows_device(self.ptr, ctypes.byref(params), c_void_p(d_out), tile_rows, rank,
                                                   nranks, c_void_p(stream or None),
                                                   c_void_p(d_segments or None)):
            raise WololoError(last_error())


def render_params(width=256, height=256, spp=1, max_depth=8, seed=0, mode=MODE_UBERSHADER_RT1, sample_offset=0,
                  time_sec=0.0) -> RenderParams:
    return RenderParams(width, height, spp, max_depth, seed, mode, sample_offset, float(time_sec))


def assemble_rows_device(d_gathered: int, d_frame: int, width: int, height: int, tile_rows: int, nranks: int,
                         stream: int = 0, band=(0, 0)):
    """Un-interleave the gathered rank buffers; `band` = (cycle, skip) of weighted bands."""
    lib = load()
    if lib.wo_assemble_rows_device_ex(c_void_p(d_gathered), c_void_p(d_frame), width, height, tile_rows, nranks,
                                      band[0], band[1], c_void_p(stream or None)):
        raise WololoError(last_error())


def srgb8_thresholds():
    """The present encode's 255 thresholds (float32 numpy array)."""
    import numpy as np
    t = (c_float * 255)()
    load().wo_srgb8_thresholds(t)
    return np.frombuffer(t, dtype=np.float32).copy()


def srgb8_encode_host(rgba):
    """(..., 4) float32 RGBA -> (...) uint32 B8G8R8A8 sRGB, the library's host encode."""
    import numpy as np
    a = np.ascontiguousarray(rgba, dtype=np.float32)
    out = np.empty(a.shape[:-1], dtype=np.uint32)
    load().wo_srgb8_encode_host(a.ctypes.data_as(c_void_p), out.ctypes.data_as(c_void_p), out.size)
    return out


def srgb8_encode_device(d_rgba: int, d_bgra8: int, pixels: int, stream: int = 0):
    if load().wo_srgb8_encode_device(c_void_p(d_rgba), c_void_p(d_bgra8), pixels, c_void_p(stream or None)):
        raise WololoError(last_error())


def denoise_params(levels=None, flags=None, k_color=None, k_normal=None, k_depth=None) -> DenoiseParams:
    """wo_denoise_params_default with the given fields replaced."""
    dp = DenoiseParams()
    load().wo_denoise_params_default(ctypes.byref(dp))
    for name, v in (("levels", levels), ("flags", flags), ("k_color", k_color), ("k_normal", k_normal),
                    ("k_depth", k_depth)):
        if v is not None:
            setattr(dp, name, v)
    return dp


def denoise_scratch_bytes(width: int, height: int, dp: DenoiseParams) -> int:
    """Bytes of device scratch wo_denoise_device needs; raises on bad arguments (the C call returns 0)."""
    n = int(load().wo_denoise_scratch_bytes(width, height, ctypes.byref(dp) if dp is not None else None))
    if n == 0:
        raise WololoError(last_error())
    return n


def denoise_host(dp: DenoiseParams, color, albedo=None, normal=None, ids=None):
    """wo_denoise_host on numpy planes: color, albedo, normal (H, W, 4) float32, ids (H, W) of
    FEATURE_IDS_FIELDS (or (H, W, 4) uint32); the optional ones may be None.  Returns (H, W, 4) float32."""
    import numpy as np
    color = np.ascontiguousarray(color, dtype=np.float32)
    h, w = color.shape[:2]
    planes = [None if a is None else np.ascontiguousarray(a) for a in (albedo, normal, ids)]
    out = np.zeros((h, w, 4), dtype=np.float32)
    ptr = [c_void_p(a.ctypes.data) if a is not None else None for a in planes]
    if load().wo_denoise_host(ctypes.byref(dp), w, h, c_void_p(color.ctypes.data), ptr[0], ptr[1], ptr[2],
                              c_void_p(out.ctypes.data)):
        raise WololoError(last_error())
    return out


def denoise_device(dp: DenoiseParams, width: int, height: int, d_color: int, d_albedo: int, d_normal: int, d_ids: int,
                   d_out: int, d_scratch: int, scratch_bytes: int, stream: int = 0):
    """wo_denoise_device on device addresses (0 = NULL), asynchronously on `stream`."""
    if load().wo_denoise_device(ctypes.byref(dp) if dp is not None else None, width, height, c_void_p(d_color or None),
                                c_void_p(d_albedo or None), c_void_p(d_normal or None), c_void_p(d_ids or None),
                                c_void_p(d_out or None), c_void_p(d_scratch or None), int(scratch_bytes),
                                c_void_p(stream or None)):
        raise WololoError(last_error())


def abi_layout(type_name: str, field: str | None = None) -> int:
    """sizeof / offsetof as the C library was compiled (wo_abi_layout); -1 if unknown."""
    v = load().wo_abi_layout(type_name.encode(), field.encode() if field else None)
    return -1 if v == ctypes.c_size_t(-1).value else int(v)


def mass_grid(lo, hi, axis: int, nu: int, nv: int, v_begin: int = 0, v_count: int | None = None) -> MassGrid:
    """A Wo_MassGrid over the clip box [lo, hi]; the whole grid unless a row range is given."""
    g = MassGrid()
    g.lo[:] = [float(x) for x in lo]
    g.hi[:] = [float(x) for x in hi]
    g.axis, g.nu, g.nv, g.v_begin = int(axis), int(nu), int(nv), int(v_begin)
    g.v_count = int(nv - v_begin if v_count is None else v_count)
    return g


def mass_grid_plan(grid: MassGrid) -> MassPlan:
    """wo_mass_grid_plan (host only): what host and kernel derive from a grid."""
    plan = MassPlan()
    if load().wo_mass_grid_plan(ctypes.byref(grid), ctypes.byref(plan)):
        raise WololoError(last_error())
    return plan


def mass_properties_from_sums(grid: MassGrid, sums: MassSums) -> MassProperties:
    """wo_mass_properties_from_sums (host only): the properties of a whole grid's sums."""
    props = MassProperties()
    if load().wo_mass_properties_from_sums(ctypes.byref(grid), ctypes.byref(sums), ctypes.byref(props)):
        raise WololoError(last_error())
    return props


def mesh_grid(lo, hi, n, iters: int = 16) -> MeshGrid:
    """A Wo_MeshGrid over the clip box [lo, hi] with n = (n0, n1, n2) cells (or one count for all three)."""
    g = MeshGrid()
    g.lo[:] = [float(x) for x in lo]
    g.hi[:] = [float(x) for x in hi]
    g.n[:] = [int(n)] * 3 if isinstance(n, int) else [int(x) for x in n]
    g.iters = int(iters)
    return g


def mesh_grid_check(grid: MeshGrid):
    """wo_mesh_grid_check (host only): the cell sizes h[3] of a good grid; raises for a bad one."""
    h = (c_float * 3)()
    if load().wo_mesh_grid_check(ctypes.byref(grid) if grid is not None else None, h):
        raise WololoError(last_error())
    return [float(x) for x in h]


def mesh_scratch_bytes(grid: MeshGrid) -> int:
    """Bytes of device scratch wo_renderer_mesh_device needs; raises for a bad grid (the C call returns 0)."""
    n = int(load().wo_mesh_scratch_bytes(ctypes.byref(grid) if grid is not None else None))
    if n == 0:
        raise WololoError(last_error())
    return n


def write_obj(path: str, vertices, quads, ids=None):
    """wo_mesh_write_obj on numpy arrays as Renderer.mesh returns them (ids None: one ungrouped list of faces)."""
    import numpy as np
    v = np.ascontiguousarray(vertices, dtype=np.dtype(MESH_VERTEX_FIELDS))
    q = np.ascontiguousarray(quads, dtype=np.uint32).reshape(-1, 4)
    i = None if ids is None else np.ascontiguousarray(ids, dtype=np.dtype(MESH_QUAD_IDS_FIELDS))
    if i is not None and len(i) != len(q):
        raise ValueError("ids: one row per quad")
    if load().wo_mesh_write_obj(os.fsencode(path), v.ctypes.data_as(c_void_p), len(v), q.ctypes.data_as(c_void_p),
                                i.ctypes.data_as(c_void_p) if i is not None else None, len(q)):
        raise WololoError(last_error())


JIT_ORIGINS = ("process", "disk", "compiled")
PEER_MODES = ("same", "dma", "staged")  # wo_dev.h WO_PEER_*


def jit_code_object(src: str, arch: str = "gfx950"):
    """(size, origin, seconds, key) of the specialised kernel's code object (wo_jit_code_object)."""
    err = ctypes.create_string_buffer(4096)
    key = ctypes.create_string_buffer(65)
    org, sec = c_int(-1), c_double(0.0)
    n = load().wo_jit_code_object(src.encode(), arch.encode(), ctypes.byref(org), ctypes.byref(sec), key, err,
                                  len(err))
    if n < 0:
        raise WololoError(err.value.decode(errors="replace"))
    return int(n), JIT_ORIGINS[org.value], sec.value, key.value.decode()


def jit_code_resources(src: str, arch: str = "gfx950"):
    """(scratch bytes per lane, static LDS bytes) of the specialised kernel's code object, from
    its kernel descriptor (wo_jit_code_resources; no GPU needed)."""
    err = ctypes.create_string_buffer(4096)
    out = (ctypes.c_uint32 * 2)()
    if load().wo_jit_code_resources(src.encode(), arch.encode(), out, err, len(err)):
        raise WololoError(err.value.decode(errors="replace"))
    return int(out[0]), int(out[1])


def jit_compile_check(src: str, arch: str = "gfx950") -> str:
    """Compile generated source with hiprtc (no GPU needed); '' on success, else the log."""
    err = ctypes.create_string_buffer(4096)
    rc = load().wo_jit_compile_check(src.encode(), arch.encode(), err, len(err))
    return "" if rc == 0 else err.value.decode(errors="replace")


class LaneBvhDesc(Structure):
    """Mirror of WoLaneBvhDesc (csrc/lane_bvh.h): all uint32."""
    _fields_ = [(n, c_uint32) for n in (
        "nprims", "nodes", "always", "root", "depth", "top", "terms", "union_only", "spheres_only", "stack16",
        "wide", "general", "term_off", "leaf_off", "gpar_off", "gnode_off", "gclip_off", "gP", "gwords", "groot")]


def lane_bvh(prog, n_recs: int, n_prims: int, mats, n_mats: int):
    """The lane tracer's BVH of a compiled program, built on the host (csrc/wo_dev.h
    wo_lane_bvh_build; no GPU needed): (descriptor, blob bytes, dynamic LDS bytes of a lane
    kernel's workgroup, (the LDS budget, the most levels of a binary tree))."""
    build = load().wo_lane_bvh_build
    build.argtypes = [POINTER(WoRec), c_uint32, c_uint32, POINTER(WoMaterial), c_uint32, POINTER(LaneBvhDesc),
                      POINTER(c_uint32), c_char_p, c_size_t, POINTER(c_size_t), c_char_p, c_size_t]
    desc, info, size, blob = LaneBvhDesc(), (c_uint32 * 3)(), c_size_t(0), ctypes.create_string_buffer(0)
    err = ctypes.create_string_buffer(256)
    for _ in range(2):  # the size, then the bytes
        if build(prog, n_recs, n_prims, mats, n_mats, ctypes.byref(desc), info, blob, len(blob), ctypes.byref(size),
                 err, len(err)):
            raise WololoError(err.value.decode(errors="replace"))
        if size.value <= len(blob):
            break
        blob = ctypes.create_string_buffer(size.value)
    return desc, blob.raw[:size.value], int(info[0]), (int(info[1]), int(info[2]))


PLAN_FIELDS = ("big_log2", "small_log2", "n_big", "tiles_x_big", "tiles_x_small", "rows_big", "workgroups")


def plan_tiles(width: int, rows: int, resident: int, band_rows: int = 0xFFFFFFFF, want_per_wg: int = 3):
    """The path tracer's launch grid for `rows` local rows of `width` pixels (csrc/wo_dev.h
    wo_plan_tiles; no GPU needed): the PLAN_FIELDS values, or None for a grid too large to launch."""
    plan = load().wo_plan_tiles
    plan.argtypes = [c_uint32] * 5 + [POINTER(c_uint32)]
    out = (c_uint32 * 7)()
    return None if plan(width, rows, resident, band_rows, want_per_wg, out) else tuple(int(v) for v in out)


def current_device() -> int:
    """The calling thread's current HIP device (csrc/wo_dev.h wo_dev_current), or -1."""
    return int(load().wo_dev_current())


def select_device(device: int):
    """Make `device` the calling thread's current HIP device (csrc/wo_dev.h wo_dev_select)."""
    if load().wo_dev_select(c_int(device)) != 0:
        raise WololoError(f"cannot select HIP device {device}")


BAND_CYCLE_MAX = 65536  # wo_scene.h WO_BAND_CYCLE_MAX


def _weighted(nranks, band):
    return nranks >= 2 and 0 < band[1] < band[0] <= BAND_CYCLE_MAX


def band_global(lb: int, rank: int, nranks: int, band=(0, 0)) -> int:
    """Mirror of wo_band_global() (wo_scene.h): the frame band of a rank's local band."""
    if not _weighted(nranks, band):
        return lb * nranks + rank
    cycle, skip = band
    full = cycle - skip
    per = full if rank == 0 else cycle
    c, j = divmod(lb, per)
    p = j * nranks + rank if j < full else full * nranks + (j - full) * (nranks - 1) + rank - 1
    return c * (cycle * nranks - skip) + p


def rank_bands(height: int, tile_rows: int, rank: int, nranks: int, band=(0, 0)) -> int:
    """Mirror of wo_rank_tile_count_ex() (wo_scene.h)."""
    tiles = (height + tile_rows - 1) // tile_rows
    if not _weighted(nranks, band):
        return (tiles - rank + nranks - 1) // nranks if rank < tiles else 0
    cycle, skip = band
    per = cycle - skip if rank == 0 else cycle
    c, rem = divmod(tiles, cycle * nranks - skip)
    return c * per + sum(1 for j in range(per) if band_global(j, rank, nranks, band) < rem)


def default_band(nranks: int):
    """The row-band weighting bench.py gives an N-rank frame: rank 0 (which also
    receives the gather, assembles and presents) sits out one round of bands in
    every `cycle`.  tools/root_step.py, csg32 1080p64, N = 8: 0:0 6.21x, 8:1 6.37x,
    12:1 6.44x; N = 4: 0:0 3.33x, 16:1 3.59x; N = 2: 0:0 1.89x, 32:1 1.92x.  Heavier
    scenes want a lighter skip (rank 0's extra work is the same milliseconds).  Round 5
    (camera-ray waves make the shares shorter, rank 0's extra work is not): N = 8 without
    the present map-back, csg32 10:1 6.69x / 5:1 6.87x, csg32_nested 7.29 / 7.66x, RTIOW
    7.45 / 7.36x (profiles/r05_root_step_nomap_n8.log)."""
    if nranks >= 8:
        return (5, 1)
    if nranks >= 4:
        return (16, 1)
    if nranks >= 2:
        return (32, 1)
    return (0, 0)


def local_rows(height: int, tile_rows: int, nranks: int, band=(0, 0)) -> int:
    """Mirror of wo_rank_local_rows_ex() (wo_scene.h)."""
    t = [rank_bands(height, tile_rows, r, nranks, band) for r in range(min(nranks, 2))]
    return max(t) * tile_rows


def global_row(lrow: int, tile_rows: int, rank: int, nranks: int, band=(0, 0)) -> int:
    lt = lrow // tile_rows
    return band_global(lt, rank, nranks, band) * tile_rows + (lrow - lt * tile_rows)
