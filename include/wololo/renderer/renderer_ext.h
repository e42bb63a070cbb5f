/*
 * wololo/renderer/renderer_ext.h -- headless / north-star extensions of the
 * renderer API.  New names only; nothing here changes renderer.h.
 *
 * The reference declares `Wo_Material` but never uses it (renderer.h:16) and has
 * no camera, sample-count or bounce controls; its per-frame inputs are the 12-byte
 * UBO {time, W, H} (renderer.c:72-80, 2133-2155).  These calls add them.
 *
 * Return convention for int-returning calls: 0 on success, negative on error;
 * wo_renderer_last_error() returns a thread-local message for the last failure.
 */
#ifndef WOLOLO_RENDERER_RENDERER_EXT_H
#define WOLOLO_RENDERER_RENDERER_EXT_H

#include <stddef.h>
#include <stdint.h>

#include "wololo/renderer/renderer.h"
#include "wololo/wo_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WO_NODE_INVALID ((Wo_Node)0xFFFFFFFFu)
#define WO_MATERIAL_INVALID ((Wo_Material)0xFFFFFFFFu)

typedef enum Wo_ShadingMode {
    WO_SHADING_UBERSHADER_RT1 = WO_MODE_UBERSHADER_RT1, /* default: the reference's image */
    WO_SHADING_DEBUG_ST = WO_MODE_DEBUG_ST,
    WO_SHADING_PATHTRACE = WO_MODE_PATHTRACE,
    WO_SHADING_NORMALS = WO_MODE_NORMALS,
} Wo_ShadingMode;

typedef struct Wo_RenderParams {
    uint32_t width, height;  /* frame size in pixels */
    uint32_t spp;            /* samples per pixel (PATHTRACE) */
    uint32_t max_depth;      /* max segments per path (PATHTRACE) */
    uint32_t seed;           /* RNG stream selector */
    uint32_t mode;           /* Wo_ShadingMode */
    uint32_t sample_offset;  /* index of the first sample (progressive rendering) */
    float time_sec;          /* UBERSHADER_RT1: time_since_start_sec */
} Wo_RenderParams;

/* Defaults: 1280x720 (or the app window), 1 spp, 8 segments, seed 0, UBERSHADER_RT1. */
void wo_render_params_default(Wo_RenderParams* params);

/* ---- materials (leaf nodes carry one; the default, id 0, is lambertian 0.5 grey) ---- */
Wo_Material wo_renderer_add_lambertian_material(Wo_Renderer* r, Wo_Vec3 albedo);
Wo_Material wo_renderer_add_metal_material(Wo_Renderer* r, Wo_Vec3 albedo, Wo_Scalar fuzz);
Wo_Material wo_renderer_add_dielectric_material(Wo_Renderer* r, Wo_Scalar refraction_index);
/* Only sphere / half-space leaves take materials.  Returns false on a bad handle. */
bool wo_renderer_set_node_material(Wo_Renderer* r, Wo_Node leaf, Wo_Material material);

/* ---- camera (RTIOW "positionable camera" with defocus blur) ---- */
void wo_renderer_set_camera(Wo_Renderer* r, Wo_Vec3 look_from, Wo_Vec3 look_at, Wo_Vec3 view_up,
                            Wo_Scalar vertical_fov_deg, Wo_Scalar aperture, Wo_Scalar focus_dist);

/* Parameters used by wo_renderer_draw_frame(); time_sec is overridden by the
 * app clock unless `pin_time` is non-zero. */
void wo_renderer_set_draw_params(Wo_Renderer* r, Wo_RenderParams const* params, int pin_time);

/* Render a whole frame into a host buffer of width*height*4 floats (RGBA,
 * row 0 = top).  Synchronous.  Includes the device->host copy. */
int wo_renderer_render_f32(Wo_Renderer* r, Wo_RenderParams const* params, float* out_rgba);

/* Render this rank's row tiles into DEVICE memory `d_out`
 * (wo_rank_local_rows(height, tile_rows, nranks) * width float4s) on HIP stream
 * `stream` (NULL = default stream), asynchronously.  Tiles are `tile_rows` rows;
 * rank r owns tiles g with g % nranks == r, stored in increasing g.  If
 * `d_segment_counter` is non-NULL, the number of traced CSG ray segments is
 * atomically added to it (uint64, device memory). */
int wo_renderer_render_rows_device(Wo_Renderer* r, Wo_RenderParams const* params, void* d_out,
                                   uint32_t tile_rows, uint32_t rank, uint32_t nranks, void* stream,
                                   unsigned long long* d_segment_counter);

/* Executed-work counters: render this rank's tiles once (synchronously, into
 * scratch memory) with the counting variant of the path kernel the renderer
 * runs -- same image, same segments -- and fill counts[WO_WORK_KINDS]
 * (wo_scene.h: segments, sphere / half-space / BOUND tests, events stored,
 * events swept, re-collects, primary segments; lane counts).  A measurement
 * aid (the counting kernel is slower); PATHTRACE / NORMALS frames only. */
int wo_renderer_count_work(Wo_Renderer* r, Wo_RenderParams const* params, uint32_t tile_rows, uint32_t rank,
                           uint32_t nranks, unsigned long long* counts);

/* Un-interleave nranks gathered local buffers (rank-major, each
 * wo_rank_local_rows(...) * width float4s) into a width*height float4 frame. */
int wo_assemble_rows_device(void const* d_gathered, void* d_frame, uint32_t width, uint32_t height,
                            uint32_t tile_rows, uint32_t nranks, void* stream);
/* The same for row bands weighted by wo_renderer_set_band_weight (buffers of
 * wo_rank_local_rows_ex(..., band_cycle, band_skip) rows). */
int wo_assemble_rows_device_ex(void const* d_gathered, void* d_frame, uint32_t width, uint32_t height,
                               uint32_t tile_rows, uint32_t nranks, uint32_t band_cycle, uint32_t band_skip,
                               void* stream);
/* Row bands of the renderer's multi-rank frames (render_rows_device, count_work
 * with nranks > 1): in every band_cycle rounds of the ranks rank 0 sits out
 * band_skip (0 = a band per rank and round, the default), so the rank that also
 * gathers, assembles and presents renders less (wo_scene.h wo_band_global).
 * -1 if 0 < band_skip >= band_cycle. */
int wo_renderer_set_band_weight(Wo_Renderer* r, uint32_t band_cycle, uint32_t band_skip);

/* ---- several GPUs per renderer ----
 * The reference renders on physical device 0 only (renderer.c:519-520).  Here
 * one renderer can split every frame over n ranks: rank i renders the
 * row-cyclic 4-row tiles g with g % n == i on HIP device (d0 + i) mod
 * visible devices (d0 = wo_renderer_device), ranks 1..n-1 copy their share to
 * d0 (peer DMA over xGMI; through pinned host memory when the pair has no peer
 * path), and d0 assembles and presents the frame.  The image is the same bit
 * for bit for every n.  n above the device count stacks ranks on one device.
 * After set_devices(n), draw_frame, render_f32, render_accumulate and
 * render_frame_device use all n ranks; render_rows_device (the caller splits
 * the frame) uses d0 only.
 * Default: WOLOLO_DEVICES=N|all (n ranks, always), else, for a renderer created
 * with an app (the demo), every visible GPU with the rank count chosen per frame
 * by workload: the reference shader, the debug view and normals frames (a few
 * microseconds of kernel) stay on d0, and a path-traced frame takes one rank
 * per WOLOLO_RANK_MIN_SAMPLES (default 4 Mi) samples, up to all of them; a
 * renderer without an app gets one rank.  WOLOLO_DEVICES=auto (every GPU) or
 * auto:N (N ranks) applies the app's workload rule to any renderer.  Returns n,
 * or -1 (last_error; the
 * renderer then keeps one rank). */
int wo_renderer_set_devices(Wo_Renderer* r, int n);
/* Ranks a frame is split over (0 for a device-less renderer). */
int wo_renderer_device_count(Wo_Renderer* r);
/* Ranks a frame with these parameters is split over (the workload rule above
 * for the app's default, else wo_renderer_device_count). */
int wo_renderer_frame_ranks(Wo_Renderer* r, Wo_RenderParams const* params);
/* How rank `rank`'s share reaches d0: 0 same device (device copy), 1 peer DMA,
 * 2 through pinned host memory (no peer path, or WOLOLO_PEER=staged); -1 for
 * rank 0 or a bad rank. */
int wo_renderer_peer_mode(Wo_Renderer* r, int rank);
/* Render a whole frame over the renderer's ranks into DEVICE memory d_frame
 * (width*height float4s on d0 = wo_renderer_device; row 0 = top), ordered on
 * HIP stream `stream` of d0 (NULL = its default stream): d_frame is written on
 * `stream` after the work queued on it before the call, and is complete when
 * `stream` reaches the point of the call's return.  The ranks render into the
 * library's own buffers on their own streams, so they may start earlier.
 * Asynchronous.  Consecutive calls alternate between two gather buffers, so
 * frame k+1 renders while frame k is gathered.  No present.  The traced CSG
 * segments are counted per rank (wo_renderer_take_segments). */
int wo_renderer_render_frame_device(Wo_Renderer* r, Wo_RenderParams const* params, void* d_frame, void* stream);
/* Segments traced by render_frame_device frames since the last call, summed
 * over the ranks (waits for their devices; the counters restart at 0). */
int wo_renderer_take_segments(Wo_Renderer* r, unsigned long long* total);

/* ---- frame pipeline and progressive rendering ----
 * The reference's draw_frame_with_renderer (renderer.c:2085-2219) ends every
 * frame with vkQueueWaitIdle (2212).  wo_renderer_draw_frame instead submits
 * frame k (asynchronous: the render on the device's render stream; the map-back
 * -- present encode and its copy to pinned host memory -- on a copy stream once
 * the render is done, so frame k+1's render never waits for frame k's copies)
 * and then waits for and presents frame k-1: the GPU renders while the host
 * presents, one frame of latency.  Presenting = the last frame below, plus a PPM
 * dump when WOLOLO_OUTPUT names a file. */
/* Wait for and present every submitted frame.  0, or -1 (last_error). */
int wo_renderer_finish(Wo_Renderer* r);
/* Host pixels of the last presented frame (RGBA float, row 0 = top; NULL
 * before the first), valid until the next draw_frame / finish.  The float frame
 * is copied from the device on the first call after a present (unless
 * wo_renderer_set_map_float asks for every frame), so a caller that only
 * presents never pays for its 16 bytes per pixel of map-back. */
float const* wo_renderer_last_frame(Wo_Renderer* r, uint32_t* width, uint32_t* height);
/* every_frame != 0: map each presented frame's float pixels back with its
 * present encode (asynchronously, on the copy stream); 0 (default): on demand. */
void wo_renderer_set_map_float(Wo_Renderer* r, int every_frame);
/* Pipeline timestamps (diagnostics): while on, each frame draw_frame presents
 * logs three times in ms after the call that turned them on -- render begin,
 * render end (both on the render stream) and map-back end (copy stream).
 * set: 0 or -1 (drains the pipeline first); frame_stamps copies up to
 * max_frames logged frames (oldest first, 3 doubles each) into out, empties the
 * log and returns how many, or -1.  The log holds 256 frames. */
int wo_renderer_set_frame_stamps(Wo_Renderer* r, int on);
int wo_renderer_frame_stamps(Wo_Renderer* r, double* out, int max_frames);
/* Present encode of the last presented frame: B8G8R8A8 sRGB, one uint32 per
 * pixel (B in the low byte) -- the reference's preferred swapchain format
 * (renderer.c:813-832) -- made on the GPU by wo_srgb8_encode_device.  Same
 * lifetime as wo_renderer_last_frame. */
uint32_t const* wo_renderer_last_frame_bgra8(Wo_Renderer* r, uint32_t* width, uint32_t* height);
/* The sRGB present encode (what the reference's B8G8R8A8_SRGB attachment does in
 * fixed function): per channel code = round-half-up(255 * srgb(clamp(v, 0, 1)))
 * with the IEC 61966-2-1 transfer function (NaN -> 0); alpha is linear.
 * wo_srgb8_thresholds gives the 255 floats the code counts (code(v) = number of
 * thresholds <= v); the device and host encodes use the same table, so they
 * agree bit for bit. */
void wo_srgb8_thresholds(float out[255]);
int wo_srgb8_encode_device(void const* d_rgba, void* d_bgra8, size_t pixels, void* stream);
void wo_srgb8_encode_host(float const* rgba, uint32_t* bgra8, size_t pixels);

/* Progressive accumulation for draw_frame (off by default): while on,
 * consecutive PATHTRACE frames with the same scene, camera and draw
 * parameters add params.spp new samples each (the sample index continues) and
 * present the mean over all of them -- bit for bit one render of that many
 * samples.  Any change starts over. */
void wo_renderer_set_progressive(Wo_Renderer* r, int on);
/* Samples per pixel in the current accumulation (0: none). */
uint32_t wo_renderer_accumulated_spp(Wo_Renderer* r);
/* Synchronous form: render params->spp more samples into the accumulation
 * (reset != 0, or different parameters / scene: start over) and write the mean
 * over all accumulated samples to out_rgba (width*height*4 floats, may be
 * NULL).  Returns the accumulated samples per pixel, or -1. */
int wo_renderer_render_accumulate(Wo_Renderer* r, Wo_RenderParams const* params, float* out_rgba, int reset);

/* Compile the node tables into the flattened program (done lazily by every
 * render call; exposed for tests).  Returns the number of records. */
int wo_renderer_compile(Wo_Renderer* r);
/* Host views of the compiled scene (valid until the next node/material change). */
WoRec const* wo_renderer_program(Wo_Renderer* r, uint32_t* n_recs, uint32_t* n_prims);
WoMaterial const* wo_renderer_materials(Wo_Renderer* r, uint32_t* n_materials);
/* Fill a WoFrame exactly as the kernels receive it (camera resolved for params). */
int wo_renderer_frame_desc(Wo_Renderer* r, Wo_RenderParams const* params, uint32_t tile_rows,
                           uint32_t rank, uint32_t nranks, WoFrame* out);

/* ---- ray queries and picking ----
 * The tracer behind the frames, asked directly: where does a ray first cross the
 * surface of the scene's solid, and which node's leaf is that.  A hit is the
 * first event after WO_T_MIN (wo_scene.h) at which the root's membership
 * changes -- the path tracer's own segment query, bit for bit. */
typedef struct Wo_Ray {      /* 32 bytes, 16-byte aligned rows: two 16 B loads per lane */
    float origin[3];
    float t_max;             /* a hit is reported only if t <= t_max; +INFINITY = unbounded */
    float dir[3];            /* used as given; expected unit length, as every ray inside the path tracer */
    uint32_t reserved;       /* ignored */
} Wo_Ray;

typedef struct Wo_RayHit {   /* 32 bytes */
    float t;                 /* ray parameter of the hit (> WO_T_MIN); +INFINITY on a miss */
    uint32_t flags;          /* WO_RAY_* */
    uint32_t leaf;           /* index of the hit leaf's record in the compiled program (wo_renderer_program) */
    Wo_Node node;            /* the sphere / half-space node that leaf was compiled from */
    float normal[3];         /* outward normal of the CSG solid at the hit (what WO_SHADING_NORMALS encodes) */
    Wo_Material material;    /* the leaf's material id, clamped as the path tracer clamps it */
} Wo_RayHit;

#define WO_RAY_HIT      1u   /* the root's membership changes at t */
#define WO_RAY_EXIT     2u   /* the event is the leaf's far boundary */
#define WO_RAY_ENTERS   4u   /* the ray enters the solid there (else it leaves it) */
#define WO_RAY_INVALID  8u   /* non-finite origin or dir, NaN t_max, or dir == 0: not traced */

/* A miss (no hit, a hit beyond t_max, an invalid ray): t = +INFINITY, leaf = node =
 * material = 0xFFFFFFFF, normal = 0, flags = 0 (WO_RAY_INVALID for an invalid ray).
 * A hit's normal is the leaf's outward normal at origin + t * dir ((P - c) / r for
 * a sphere, n for a half-space), negated under WO_RAY_EXIT and negated again
 * without WO_RAY_ENTERS. */

/* Trace n rays in DEVICE memory into n hits in device memory, on the renderer's
 * device (wo_renderer_device; whatever wo_renderer_set_devices says),
 * asynchronously on HIP stream `stream` (NULL = the default stream), ordered as
 * wo_renderer_render_rows_device is.  Both buffers are 16-byte aligned.  An
 * edited scene is compiled and uploaded first, as by a render.  n = 0 launches
 * nothing.  0, or -1 (last_error; always for a device-less renderer). */
int wo_renderer_trace_rays_device(Wo_Renderer* r, Wo_Ray const* d_rays, Wo_RayHit* d_hits, size_t n, void* stream);
/* The same from and to host memory (synchronous; includes both copies). */
int wo_renderer_trace_rays(Wo_Renderer* r, Wo_Ray const* rays, Wo_RayHit* hits, size_t n);
/* The ray a WO_SHADING_NORMALS frame of params' size traces through pixel (x, y)
 * (row 0 = top) with the current camera: the pixel centre, no lens offset,
 * t_max = +INFINITY.  Host arithmetic, no device needed.  -1 outside the frame. */
int wo_renderer_pixel_ray(Wo_Renderer* r, Wo_RenderParams const* params, uint32_t x, uint32_t y, Wo_Ray* out);
/* What lies under pixel (x, y): pixel_ray, then a one-ray trace_rays. */
int wo_renderer_pick(Wo_Renderer* r, Wo_RenderParams const* params, uint32_t x, uint32_t y, Wo_RayHit* out);
/* Per record of the compiled program (wo_renderer_program) the node it was
 * compiled from: the sphere / half-space node for WO_LEAF_* records (every
 * instance of a node used several times names that node), WO_NODE_INVALID for
 * all others.  Valid until the next node / material change. */
Wo_Node const* wo_renderer_program_nodes(Wo_Renderer* r, uint32_t* n_recs);
/* Kernel of the ray queries (results are identical; only speed differs):
 *   AUTO         LANES where it applies, else INTERPRETER;
 *   INTERPRETER  the postfix-program interpreter, one wave walking the program
 *                for its 64 rays (any scene; best for coherent rays);
 *   LANES        per-lane BVH traversal (union-only scenes; others fall back to
 *                the interpreter).
 * The scene-specialised kernel is not used for ray queries. */
typedef enum Wo_RayTracer { WO_RAY_TRACER_AUTO = 0, WO_RAY_TRACER_INTERPRETER = 1, WO_RAY_TRACER_LANES = 2 } Wo_RayTracer;
void wo_renderer_set_ray_tracer(Wo_Renderer* r, Wo_RayTracer tracer);
/* Which kernel the last ray launch used: "interpreter", "lanes" or "none". */
char const* wo_renderer_ray_path(Wo_Renderer* r);

/* ---- ray span queries (ray classification) and point classification ----
 * Every interval of a ray that lies inside the solid, and whether a point does.
 * The crossings of a ray are the events, in the tracer's key order (t, primitive
 * ordinal, entry before exit), at which the root's membership changes, with
 * WO_T_MIN < t <= t_max.  Crossing 0 is what wo_renderer_trace_rays reports for the
 * ray; the later ones come from the same sweep carried on -- no restart, no new
 * origin.  Coincident surfaces are decided by the key order alone, one event at a
 * time, so a zero-length span (two crossings of equal t) is reported, not merged. */
#define WO_RAY_INSIDE    16u  /* Wo_RaySpans.flags: the root contains the ray's point at WO_T_MIN */
#define WO_RAY_TRUNCATED 32u  /* Wo_RaySpans.flags: count > max_crossings */

typedef struct Wo_RayCrossing {  /* 16 bytes */
    float t;                 /* WO_T_MIN < t <= t_max */
    uint32_t flags;          /* WO_RAY_HIT | WO_RAY_EXIT? | WO_RAY_ENTERS?, as Wo_RayHit.flags */
    uint32_t leaf;           /* record index in the compiled program */
    Wo_Node node;            /* the node that leaf was compiled from */
} Wo_RayCrossing;

typedef struct Wo_RaySpans {     /* 16 bytes per ray */
    uint32_t count;          /* all crossings in (WO_T_MIN, t_max], however many were stored */
    uint32_t flags;          /* WO_RAY_INSIDE, WO_RAY_TRUNCATED, WO_RAY_INVALID */
    float length;            /* total length of the ray inside the solid within (WO_T_MIN, t_max] */
    uint32_t stored;         /* min(count, max_crossings) */
} Wo_RaySpans;

/* `length` is summed in fp32, one rounding per operation, in sweep order: len = 0,
 * t_in = WO_T_MIN; a crossing that enters sets t_in = t; one that leaves adds
 * (t - t_in); after the last crossing, a ray that is inside with t_max > t_in adds
 * (t_max - t_in), which is +INFINITY for t_max = +INFINITY.  WO_RAY_INSIDE is also
 * right for a ray without any event (one inside a lone half-space).  An invalid ray
 * (as for trace_rays) gets count = stored = 0, length = 0, flags = WO_RAY_INVALID.
 *
 * n Wo_Ray at d_rays -> n Wo_RaySpans at d_spans and the crossings at d_crossings,
 * CROSSING-MAJOR: ray i's k-th crossing is d_crossings[k * n + i], k < stored (a
 * wave's k-th store is 64 consecutive rows); rows with k >= stored are not written.
 * count and length cover all crossings whatever max_crossings is, so max_crossings =
 * 0 (d_crossings may then be NULL) is the thickness query: 16 bytes written per ray.
 * Device memory, 16-byte aligned, asynchronous on `stream`; everything else as
 * wo_renderer_trace_rays_device.  Always the interpreter's sweep (ray_path then
 * says "interpreter"); wo_renderer_set_ray_tracer has no say. */
int wo_renderer_trace_spans_device(Wo_Renderer* r, Wo_Ray const* d_rays, Wo_RaySpans* d_spans,
                                   Wo_RayCrossing* d_crossings, size_t n, uint32_t max_crossings, void* stream);
/* The same from and to host memory (synchronous; includes the copies).  Crossing
 * rows the query does not write keep the caller's content. */
int wo_renderer_trace_spans(Wo_Renderer* r, Wo_Ray const* rays, Wo_RaySpans* spans, Wo_RayCrossing* crossings,
                            size_t n, uint32_t max_crossings);

#define WO_POINT_INSIDE  1u
#define WO_POINT_INVALID 8u   /* a non-finite coordinate: not classified */
/* Is each of n points (float4 rows x, y, z, w; w ignored; 16-byte aligned) inside
 * the solid?  Every leaf is evaluated in fp32, one rounding per operation: a sphere
 * contains p iff ((g.x g.x + g.y g.y) + g.z g.z) <= r^2 with g = p - c, a half-space
 * iff ((n.x p.x + n.y p.y) + n.z p.z) <= h; a primitive is the AND of its members,
 * the operators apply as in wo_scene.h, and an empty scene contains nothing.
 * d_out[i] = WO_POINT_INSIDE, 0, or WO_POINT_INVALID.  Asynchronous on `stream`,
 * otherwise as wo_renderer_trace_rays_device. */
int wo_renderer_classify_points_device(Wo_Renderer* r, float const* d_points, uint32_t* d_out, size_t n, void* stream);
/* The same from and to host memory (synchronous; includes both copies). */
int wo_renderer_classify_points(Wo_Renderer* r, float const* points, uint32_t* out, size_t n);

/* ---- mass properties (volume, centre of mass, inertia) by ray-grid integration ----
 * A grid of nu x nv parallel rays along +axis through a clip box; every span of a ray
 * inside the solid is integrated as it is swept.  The device accumulates EXACT
 * integers, so the sums do not depend on launch geometry, wave order or how many
 * calls or devices share a grid, and a CPU reference can match them bit for bit. */
typedef struct Wo_MassGrid {        /* 48 bytes */
    float lo[3], hi[3];             /* clip box: finite, lo < hi on every axis */
    uint32_t axis;                  /* 0, 1, 2: rays run along +axis; u = (axis+1)%3, v = (axis+2)%3 */
    uint32_t nu, nv;                /* cells (= rays) across u and v, 1 .. 32768 each */
    uint32_t v_begin, v_count;      /* rows j in [v_begin, v_begin + v_count) of the nv rows; v_count >= 1 */
    uint32_t reserved;              /* 0 */
} Wo_MassGrid;
#define WO_MASS_MAX_CELLS 32768u

typedef struct Wo_MassPlan {        /* what host and kernel derive from a grid; all fp32 ops single-rounded */
    float o_axis, pad, t_max, scale;/* ray origin on the axis, 0x1p-9f, pad + (hi-lo)[axis], 2^k */
    int32_t k;
    uint32_t q0, q1;                /* Q(pad), Q(t_max) */
    float u0, hu, v0, hv;           /* lo[u], (hi[u]-lo[u]) / (float)(2*nu); same for v */
} Wo_MassPlan;

typedef struct Wo_MassSums {        /* 192 bytes, exact */
    uint64_t lo[10], hi[10];        /* sum s = lo[s] + hi[s] * 2^32 */
    uint64_t rays, rays_hit, crossings, reserved;
} Wo_MassSums;

typedef struct Wo_MassProperties {
    double volume, centroid[3], inertia[9];  /* unit density, about the centroid, row-major, off-diagonals -int(ab) */
    double projected_area;                   /* rays_hit * cell area */
    double cell[3];                          /* 2hu, 2hv, 2^-k */
    uint64_t rays, crossings;
} Wo_MassProperties;

/* The plan.  pad = 0x1p-9f (above WO_T_MIN, so a surface on the box's near face is a
 * crossing); o_axis = lo[axis] - pad; t_max = pad + (hi[axis] - lo[axis]), the
 * difference and the sum one fp32 operation each.  frexpf(t_max) = (m, e): k = 20 - e,
 * scale = 2^k; |k| > 100 is rejected.  Q(t) = (uint32) rintf(t * scale), half to even;
 * scale is a power of two, so the product is exact and Q(t) <= 2^20 for t <= t_max.
 * u0 = lo[u], hu = (hi[u] - lo[u]) / (float)(2 nu) (two operations); v likewise.
 * -1 with wo_renderer_last_error for a bad grid: a non-finite value (t_max included),
 * lo >= hi, axis > 2, a count of 0 or above 32768, v_count = 0, a row range that
 * leaves nv, or reserved != 0.  Host arithmetic, no device needed.
 *
 * Ray (i, j), 0 <= i < nu, j a row of the range: origin o_axis on the axis,
 * u0 + (float)(2i+1) * hu on u and v0 + (float)(2j+1) * hv on v (a product and a sum,
 * not contracted), direction +e_axis, t_max the plan's.  Its crossings are exactly
 * those wo_renderer_trace_spans reports for that Wo_Ray.
 *
 * Per ray, with c(t) = min(max(Q(t), q0), q1): qa = q0 if the ray carries
 * WO_RAY_INSIDE; a crossing that enters sets qa = c(t); one that leaves at
 * qb = c(t) adds m0 += qb - qa, m1 += qb^2 - qa^2, m2 += qb^3 - qa^3; a ray still
 * inside after its last crossing closes at qb = q1 (an unbounded half-space, a solid
 * cut by the far face).  The box is therefore a true clip box: the part of a span
 * nearer than pad clamps to q0, the part beyond t_max is never swept.
 *
 * With i' = 2i+1 and j' = 2j+1 (j counted in the whole grid), the ten sums over the
 * rays are, in order: m0, m0 i', m0 j', m1, m0 i'^2, m0 j'^2, m2, m0 i' j', m1 i',
 * m1 j'.  Every ray's term x is below 2^63 (m2 <= 2^60) and adds x & 0xFFFFFFFF to
 * lo[s] and x >> 32 to hi[s]: up to 2^31 rays accumulated into one Wo_MassSums
 * cannot overflow a limb.  rays counts every ray of the row range, rays_hit those
 * with m0 > 0, crossings sums the rays' Wo_RaySpans.count; reserved is not touched. */
int wo_mass_grid_plan(Wo_MassGrid const* grid, Wo_MassPlan* plan);
/* The properties of the column model, in double, from (partial sums added up to) a
 * whole grid: each ray stands for a column of 2hu x 2hv.  h = 2^-k, A = (2hu)(2hv),
 * S0..S9 the ten sums (lo + hi 2^32, exact in unsigned __int128):
 *   volume V = A h S0;  local means  u = hu S1/S0,  v = hv S2/S0,  t = (h/2) S3/S0;
 *   centroid (lo[u] + u, lo[v] + v, o_axis + t), permuted to x, y, z;
 *   second moments about the local origin
 *     Euu = A h (hu^2 S4 + hu^2/3 S0), Evv likewise with S5, Ett = A h^3/3 S6,
 *     Euv = A h hu hv S7, Eut = A h^2/2 hu S8, Evt = A h^2/2 hv S9;
 *   central moments Cab = Eab - V a b;  inertia = trace(C) 1 - C.
 * S0 = 0: volume 0, the centroid is the box's centre, the inertia 0.
 * projected_area = rays_hit A; cell = (2hu, 2hv, h).  -1 for a bad grid. */
int wo_mass_properties_from_sums(Wo_MassGrid const* grid, Wo_MassSums const* sums, Wo_MassProperties* out);
/* Adds the sums of the grid's row range into *d_sums: device memory, 8-byte
 * aligned, zeroed by the caller before the first part.  Several row ranges, or
 * several renderers on several devices, may so accumulate one grid: the sum of the
 * parts is the whole, bit for bit.  Asynchronous on `stream` and ordered as
 * wo_renderer_trace_spans_device is (an edited scene is compiled and uploaded
 * first); always the interpreter's sweep.  -1 on a device-less renderer. */
int wo_renderer_mass_sums_device(Wo_Renderer* r, Wo_MassGrid const* grid, Wo_MassSums* d_sums, void* stream);
/* The host form: zeroes a device buffer, runs the row range the grid names, copies
 * the sums back (also to *sums_or_null) and finalises them (synchronous). */
int wo_renderer_mass_properties(Wo_Renderer* r, Wo_MassGrid const* grid, Wo_MassProperties* out,
                                Wo_MassSums* sums_or_null);

/* ---- first-hit feature buffers (albedo, normal, depth, coverage, ids) of a frame ----
 * The guide layers of a path-traced frame, made from the rays that frame shoots: per
 * pixel the mean first-hit albedo, facing normal and depth over the frame's own camera
 * samples (sub-pixel jitter and lens offsets included, so the planes line up with the
 * noisy frame at edges and under defocus), the coverage, and the node under the pixel
 * centre.  A separate pass of spp + 1 camera-ray traces per pixel; exact 32.32 sums make
 * every value independent of launch geometry, and a CPU reference matches bit for bit.
 *
 * For Wo_RenderParams {width W, height H, spp, seed, sample_offset}, mode =
 * WO_SHADING_PATHTRACE (max_depth and time_sec are ignored), sample s, 0 <= s < spp, of
 * pixel (x, y) (row 0 = top) is the camera ray of the path tracer (oracle.c shade_pixel),
 * every operation fp32 and rounded once, in this order:
 *   rng = pcg(y W + x ^ pcg((sample_offset + s) ^ pcg(seed)));  jx, jy = two draws of rng;
 *   u = ((float)x + jx) * inv_width;  v = ((float)(H - 1 - y) + jy) * inv_height;
 *   off = 0, or with lens_radius > 0 two more draws: rad = sqrt_pt(draw), (s, c) =
 *     sincos_turn(draw), rx = lens_radius * (rad c), ry = lens_radius * (rad s),
 *     off = cam.u * rx + cam.v * ry;
 *   o = origin + off;  d = normalize(((lower_left + u horizontal) + v vertical) - origin - off)
 * with the camera as wo_renderer_frame_desc resolves it.  Its first hit h is the tracer's
 * segment query (what wo_renderer_trace_rays reports with t_max = +INFINITY), so a
 * sample's hit / miss and t are those of the path-traced frame's first segment for the
 * same parameters.  With L the hit member's leaf record:
 *   facing normal ns: the leaf's outward normal at o + t d, negated for WO_RAY_EXIT and
 *     negated again without WO_RAY_ENTERS -- Wo_RayHit.normal;
 *   albedo a: m = materials[L.u0 < n_materials ? L.u0 : 0]; m.albedo for a lambertian or
 *     a metal, (1, 1, 1) for a dielectric;
 *   a miss: a = the sky's colour along d (the radiance that sample adds to the frame),
 *     ns = 0, no depth.
 * With Q(v) = (int64)((double)v * 2^32) (0 for |v| >= 2^20 or NaN) and M(sum, n) =
 * (float)(((double)sum * 2^-32) / (double)n), the frame's own accumulation, and `hits` the
 * samples that hit:
 *   plane WO_FEATURE_ALBEDO, float4: rgb[i] = M(sum_s Q(a_i), spp);  w = coverage =
 *     (float)((double)hits / (double)spp);
 *   plane WO_FEATURE_NORMAL, float4: xyz[i] = M(sum_s Q(ns_i), spp) -- misses add 0, so
 *     its length falls with the coverage;  w = depth = M(sum_{hits} Q(t), hits), or
 *     +INFINITY when hits = 0;
 *   plane WO_FEATURE_IDS, Wo_FeatureIds: the pixel-CENTRE ray, the one
 *     wo_renderer_pixel_ray returns (no jitter, no lens, t_max = +INFINITY): node, leaf
 *     and material as in Wo_RayHit, flags = its WO_RAY_* (0xFFFFFFFF x 3 and flags = 0 on
 *     a miss) -- wo_renderer_pick(params, x, y) field for field, for every pixel at once;
 *     one more ray per pixel, the same for every spp and sample_offset.
 * The sums are exact while a pixel's sum of |v| stays below 2^31 (as the frame's are).
 * Progressive accumulation is not kept: average batches of disjoint sample_offset
 * ranges in float. */
#define WO_FEATURE_ALBEDO 0u   /* rgb = mean first-hit albedo (sky on a miss), w = coverage */
#define WO_FEATURE_NORMAL 1u   /* xyz = mean facing normal, w = mean hit depth (+inf: no hit) */
#define WO_FEATURE_IDS    2u   /* Wo_FeatureIds of the pixel-centre ray */
#define WO_FEATURE_PLANES 3u
typedef struct Wo_FeatureIds {   /* 16 bytes */
    Wo_Node node;
    uint32_t leaf;
    Wo_Material material;
    uint32_t flags;
} Wo_FeatureIds;

/* This rank's rows of the three planes into DEVICE memory d_out (16-byte aligned):
 * plane p of the rank-local pixel (lrow, x) is the 16-byte row p * plane_stride +
 * lrow * width + x.  plane_stride counts 16-byte rows and is at least local_rows * width,
 * local_rows = wo_rank_local_rows[_ex](height, tile_rows, nranks[, band weight]); rows of
 * a plane beyond local_rows * width are not written, nor are local rows past the frame's
 * last row.  The rank's rows and their order are exactly those of
 * wo_renderer_render_rows_device with the same tile_rows, rank and nranks (band weights
 * included), so each plane is a float4 frame that wo_assemble_rows_device[_ex], a gather
 * over ranks and wo_srgb8_encode_device take unchanged.  Asynchronous on `stream`, on the
 * renderer's device, after an edited scene is compiled and uploaded, as the ray queries.
 * The kernel is the ray queries' (wo_renderer_set_ray_tracer; wo_renderer_ray_path and
 * wo_renderer_lanes_info report it); the specialised kernel is not used.
 * -1 with wo_renderer_last_error, checked in this order before the device is touched:
 * params == NULL; width, height or spp == 0; mode != WO_SHADING_PATHTRACE; nranks == 0,
 * rank >= nranks or tile_rows == 0; a short plane_stride; a NULL or misaligned buffer;
 * then a device-less renderer. */
int wo_renderer_render_features_device(Wo_Renderer* r, Wo_RenderParams const* params, void* d_out, size_t plane_stride,
                                       uint32_t tile_rows, uint32_t rank, uint32_t nranks, void* stream);
/* The whole frame on one rank into HOST memory: 3 * width * height 16-byte rows, the
 * planes contiguous (plane_stride = width * height), `out` 16-byte aligned.
 * Synchronous; includes the copy.  Uses the renderer's device only, whatever
 * wo_renderer_set_devices says. */
int wo_renderer_render_features(Wo_Renderer* r, Wo_RenderParams const* params, void* out);

/* ---- edge-avoiding a-trous denoiser guided by the feature buffers ----
 * The consumer of the planes above: `levels` passes of a 5x5 B3-spline stencil whose taps
 * are 2^i pixels apart in pass i, each tap weighted down by how far its colour, normal and
 * depth are from the centre's.  No transcendental function: every operation below is fp32
 * and rounded once, nothing is contracted, and 1.0f / x is the correctly rounded reciprocal,
 * so the device form, the host form and a CPU restatement agree bit for bit.
 *
 * Planes: width * height 16-byte rows each, row 0 at the top, 16-byte aligned.  `color` is a
 * frame as wo_renderer_render_rows_device (assembled) or wo_renderer_render_frame_device
 * leaves it; `albedo` and `normal` are planes WO_FEATURE_ALBEDO and WO_FEATURE_NORMAL (the
 * normal plane's w is the depth, +INFINITY where nothing was hit); `ids` is plane
 * WO_FEATURE_IDS.  albedo may be NULL only without WO_DENOISE_DEMODULATE, normal only when
 * k_normal == 0 && k_depth == 0, ids only without WO_DENOISE_STOP_AT_NODES.
 *
 *   clampf(v, lo, hi):  t = v > lo ? v : lo;  t < hi ? t : hi           (a NaN becomes lo)
 *   E(d2, k):           x = 1.0f - d2 * k;  m = x > 0 ? x : 0;  m * m   (a NaN gives 0)
 *   |d|^2:              (d.x d.x + d.y d.y) + d.z d.z
 * Demodulation (WO_DENOISE_DEMODULATE; per pixel and channel i): a'_i = clampf(albedo_i,
 * 0x1p-7f, 0x1p20f) and c_i = color_i * (1.0f / a'_i); otherwise c = color.rgb.
 * Depth (per pixel): z = normal.w; fin = z < INFINITY (false for a NaN); rz = 1.0f /
 * clampf(z, 0x1p-20f, 0x1p20f).
 * Pass i = 0 .. levels-1 reads the image c and writes c', with s = 1 << i and kc = k_color *
 * (float)(1u << 2i).  For the centre p = (x, y): sum = (0, 0, 0), wsum = 0; then dy = -2..2
 * (outer) and dx = -2..2 (inner), the tap q = (x + dx s, y + dy s) in signed arithmetic; a q
 * outside the frame is skipped.  h = H[|dx|] * H[|dy|], H = {0.375f, 0.25f, 0.0625f}.  The
 * centre tap has w = h.  Any other tap starts with e = 1.0f and applies the enabled terms in
 * this order:
 *   k_color > 0:   e *= E(|c_q - c_p|^2, kc);
 *   k_normal > 0:  e *= E(|n_q - n_p|^2, k_normal), n = normal.xyz as stored;
 *   k_depth > 0:   both fin: rel = (z_q - z_p) * rz_p, e *= E(rel * rel, k_depth);
 *                  neither fin: e unchanged;  exactly one fin: e = 0;
 *   WO_DENOISE_STOP_AT_NODES: ids_q.node != ids_p.node sets e = 0;
 * and w = h * e.  A tap with !(w > 0) is skipped entirely (a non-finite neighbour that a term
 * rejects never reaches the sum); otherwise sum_i += w * c_q,i (a product, then a sum) and
 * wsum += w.  c'_p = sum * (1.0f / wsum); the centre tap alone gives wsum >= 9/64.
 * After the last pass out.rgb = c * a' with WO_DENOISE_DEMODULATE, else c; out.w is color.w,
 * copied bit for bit.  Every reciprocal's argument lies in [2^-20, 2^20]. */
#define WO_DENOISE_DEMODULATE    1u  /* divide by the first-hit albedo before filtering, multiply after */
#define WO_DENOISE_STOP_AT_NODES 2u  /* a tap whose Wo_FeatureIds.node differs from the centre's gets weight 0 */
#define WO_DENOISE_MAX_LEVELS    8u
typedef struct Wo_DenoiseParams {   /* 24 bytes */
    uint32_t levels;                /* 1 .. 8 a-trous iterations; iteration i uses step 2^i */
    uint32_t flags;                 /* WO_DENOISE_* ; other bits rejected */
    float k_color, k_normal, k_depth; /* finite, >= 0; 0 switches the term off */
    uint32_t reserved;              /* 0 */
} Wo_DenoiseParams;
#define WO_DENOISE_MAX_EXTENT 32768u
/* 5 levels, WO_DENOISE_DEMODULATE, k_color 0.25f, k_normal 4.0f, k_depth 100.0f. */
void wo_denoise_params_default(Wo_DenoiseParams* dp);
/* Bytes of device scratch wo_denoise_device needs for a width x height frame: the ping-pong
 * working images, width * height * 16 bytes for one level and twice that for more.  0 on bad
 * arguments (wo_renderer_last_error names the first). */
size_t wo_denoise_scratch_bytes(uint32_t width, uint32_t height, Wo_DenoiseParams const* dp);
/* The filter on DEVICE memory: library-level, like wo_srgb8_encode_device -- on the current HIP
 * device, asynchronously on `stream` (NULL = the default stream).  Allocates nothing: d_scratch
 * holds at least wo_denoise_scratch_bytes bytes (more is accepted; only that many are written).
 * d_out and d_scratch must not overlap an input or each other.  A prologue kernel writes the
 * (demodulated) working image, one kernel per level filters it, the last one into d_out.
 * Per level the kernel either reads its taps from global memory or stages a workgroup's tile
 * and halo in LDS; WOLOLO_DENOISE_FORM = lds | direct | auto (default) picks, `lds` falling
 * back to `direct` at a step whose tile no longer fits.  The results do not depend on it.
 * -1 with wo_renderer_last_error naming the argument, checked in this order before the device
 * is touched: NULL params; levels outside 1 .. 8; unknown flag bits; reserved != 0; a negative
 * or non-finite k_*; width or height 0 or above 32768; a required plane (color, out, scratch,
 * and albedo / normal / ids as above) NULL; a misaligned pointer; out or scratch overlapping an
 * input or each other; short scratch. */
int wo_denoise_device(Wo_DenoiseParams const* dp, uint32_t width, uint32_t height, void const* d_color,
                      void const* d_albedo, void const* d_normal, void const* d_ids, void* d_out, void* d_scratch,
                      size_t scratch_bytes, void* stream);
/* The same filter in host C on host memory, bit for bit; needs no device and no scratch.  The
 * same checks in the same order. */
int wo_denoise_host(Wo_DenoiseParams const* dp, uint32_t width, uint32_t height, void const* color,
                    void const* albedo, void const* normal, void const* ids, void* out);
/* A denoised frame into HOST memory (width * height * 4 floats): the WO_SHADING_PATHTRACE frame
 * of `params` (params->mode must say so), that frame's feature planes, wo_denoise_device with
 * `dp_or_null` (NULL = the defaults) and one copy to the host, in order on one stream of the
 * renderer's own device (whatever wo_renderer_set_devices says, as render_features).
 * Synchronous.  Bit for bit wo_denoise_host applied to wo_renderer_render_f32's and
 * wo_renderer_render_features' outputs.  -1 for NULL params or out_rgba, bad denoise
 * parameters (as above), a width, height or spp of 0, another mode; then for a device-less
 * renderer. */
int wo_renderer_render_denoised(Wo_Renderer* r, Wo_RenderParams const* params, Wo_DenoiseParams const* dp_or_null,
                                float* out_rgba);

/* ---- surface mesh of the solid (naive surface nets on a uniform grid) ----
 * The solid itself, clipped to a box, as a closed quad mesh: one vertex per grid cell the
 * surface passes through, one quad per grid edge it crosses.  Everything is defined by point
 * classification (above: BOUND records ignored), every operation is fp32 and rounded once,
 * nothing is contracted, the division is correctly rounded; the order of every row is fixed,
 * so nothing depends on launch geometry and a CPU restatement matches bit for bit.
 *
 * Grid.  h[a] = (hi[a] - lo[a]) / (float)n[a].  Corner (i, j, k), 0 <= i <= n[0] and likewise
 * j, k, has coordinate c_a(i) = lo[a] + (float)i * h[a] (a product, then a sum).  Corners are
 * numbered (k (n1+1) + j)(n0+1) + i, cells (k n1 + j) n0 + i.  wo_mesh_grid_check returns -1
 * with wo_renderer_last_error naming the first failing check, in this order: a NULL grid; a
 * non-finite bound; lo >= hi; a count outside 2 .. WO_MESH_MAX_CELLS; iters > 24; flags != 0;
 * reserved != 0; a non-finite h, or h <= 0.  Host arithmetic, no device needed.
 *
 * Inside.  A corner is inside iff it is not on the grid's outermost layer (0 < i < n[0],
 * likewise j and k) and point classification calls it WO_POINT_INSIDE.  So the mesh is that of
 * the solid clipped to the box: an unbounded half-space, or a solid cut by a face of the box,
 * is closed there by cap quads.
 *
 * Crossing of a grid edge.  The edge along axis a from corner C to C + e_a is taken when the
 * two inside bits differ.  ta = c_a(C), tb = c_a(C + e_a), sa = the inside bit of C; `iters`
 * times: tm = 0.5f * (ta + tb); sm = the plain classification (nothing forced: the point is
 * not a corner) of the edge's point with coordinate a replaced by tm; sm == sa sets ta = tm,
 * else tb = tm.  The crossing is x = 0.5f * (ta + tb).
 *
 * Ids of that edge's quad.  A = the plain classification at the final ta, B at the final tb.
 * A == B (only possible when the outside end is a forced corner): a cap, leaf = node =
 * material = 0xFFFFFFFF and WO_MESH_QUAD_CAP.  Otherwise leaf is the first leaf record, in
 * program order, whose own test (v <= f[3], as point classification states it) differs between
 * the two points -- one exists, the root being a function of the leaf tests -- and node and
 * material are that leaf's as in Wo_RayHit.  Coincident surfaces are thereby decided by record
 * order.  flags = a | WO_MESH_QUAD_POSITIVE (sa set) | WO_MESH_QUAD_CAP.
 *
 * Vertices.  A cell with any of its 12 edges taken is active and gets one vertex; vertices are
 * ordered by cell number, which vertex.cell holds.  Per coordinate the position is a sum from
 * +0, in this order: a = 0, 1, 2 with u = (a+1)%3, v = (a+2)%3; dv = 0, 1; du = 0, 1; the edge
 * along a from the cell's corner offset by du e_u + dv e_v, if taken, adds the point whose
 * coordinate a is the crossing and whose u and v are that corner's.  Then each sum is divided
 * by (float)count.
 *
 * Quads.  One per taken edge, ordered by (corner number of the lower corner) * 3 + a.  With the
 * lower corner's cell coordinates as origin the four cells are at (u, v) offsets (-1,-1),
 * (0,-1), (0,0), (-1,0) (all exist: a taken edge has an interior end); v[0..3] holds their
 * vertex indices in that order when the lower corner is inside (the normal points along +a),
 * else reversed.  The surface is closed and faces outward: every directed edge p->q of the
 * quads occurs exactly as often as q->p.
 *
 * Counts and truncation.  d_counts always gets the full counts; rows >= max_* are not written;
 * indices always use the full numbering; WO_MESH_TRUNCATED is set when either maximum was
 * exceeded.  With max_vertices == 0 && max_quads == 0 the three buffers may be NULL: the
 * counting passes and the edge pass (cap_quads is its count) run, nothing is emitted. */
#define WO_MESH_MAX_CELLS 1024u
#define WO_MESH_MAX_ITERS 24u
typedef struct Wo_MeshGrid {      /* 48 bytes */
    float lo[3], hi[3];           /* clip box: finite, lo < hi on every axis */
    uint32_t n[3];                /* cells per axis, 2 .. WO_MESH_MAX_CELLS */
    uint32_t iters;               /* bisection steps per crossing edge, 0 .. 24 */
    uint32_t flags;               /* none defined: must be 0 */
    uint32_t reserved;            /* 0 */
} Wo_MeshGrid;
typedef struct Wo_MeshVertex { float p[3]; uint32_t cell; } Wo_MeshVertex;     /* 16 bytes */
typedef struct Wo_MeshQuad   { uint32_t v[4]; } Wo_MeshQuad;                   /* 16 bytes */
typedef struct Wo_MeshQuadIds { uint32_t leaf; Wo_Node node; Wo_Material material; uint32_t flags; } Wo_MeshQuadIds; /* 16 bytes */
typedef struct Wo_MeshCounts { uint32_t vertices, quads, cap_quads, flags; } Wo_MeshCounts;  /* 16 bytes */
#define WO_MESH_TRUNCATED     1u  /* counts.flags: vertices > max_vertices or quads > max_quads */
#define WO_MESH_QUAD_AXIS     3u  /* ids.flags & 3: axis of the grid edge the quad is dual to */
#define WO_MESH_QUAD_POSITIVE 4u  /* the edge's lower corner is inside: the quad faces +axis */
#define WO_MESH_QUAD_CAP      8u  /* the quad closes the solid at the clip box, no leaf */

/* The checks above; h_out (may be NULL) gets the three cell sizes of a good grid. */
int wo_mesh_grid_check(Wo_MeshGrid const* grid, float h_out[3]);
/* Bytes of device scratch wo_renderer_mesh_device needs: about 12.7 bytes per corner (one
 * inside bit, four mask bits and a count per corner, one crossing per edge).  0 for a bad grid. */
size_t wo_mesh_scratch_bytes(Wo_MeshGrid const* grid);
/* The mesh into DEVICE memory: asynchronous on `stream`, on the renderer's device only, ordered
 * and uploaded as wo_renderer_trace_rays_device (an edited scene is compiled and uploaded
 * first).  Allocates nothing and never waits for the host.  Every buffer is 16-byte aligned;
 * d_quad_ids may be NULL; d_scratch holds at least wo_mesh_scratch_bytes(grid) bytes (more is
 * accepted, only that many are used) and must not overlap an output.  -1 with
 * wo_renderer_last_error, checked in this order before the device is touched: the grid (as
 * wo_mesh_grid_check); a NULL d_counts or d_scratch; a NULL d_vertices with max_vertices > 0 or
 * a NULL d_quads with max_quads > 0; a misaligned buffer; short scratch; then a device-less
 * renderer.  wo_renderer_ray_path is left as it was, as by point classification. */
int wo_renderer_mesh_device(Wo_Renderer* r, Wo_MeshGrid const* grid, Wo_MeshVertex* d_vertices, uint32_t max_vertices,
                            Wo_MeshQuad* d_quads, Wo_MeshQuadIds* d_quad_ids, uint32_t max_quads,
                            Wo_MeshCounts* d_counts, void* d_scratch, size_t scratch_bytes, void* stream);
typedef struct Wo_Mesh { Wo_MeshVertex* vertices; Wo_MeshQuad* quads; Wo_MeshQuadIds* quad_ids; Wo_MeshCounts counts; } Wo_Mesh;
/* The whole mesh into HOST arrays the library allocates (synchronous): a counts-only pass, the
 * allocation, then the full pass, through the renderer's staging buffer and stream.  Release
 * the arrays with wo_mesh_free, which leaves NULLs and zero counts. */
int wo_renderer_mesh(Wo_Renderer* r, Wo_MeshGrid const* grid, Wo_Mesh* out);
void wo_mesh_free(Wo_Mesh* mesh);
/* Wavefront OBJ of a mesh in host memory (pure host code): "v" lines with %.9g (a float
 * round-trips), "f" lines of 1-based quads.  With ids the faces are grouped "g node_<id>" in
 * ascending node order, then "g cap"; quad order is kept inside a group.  0, or -1 (last_error). */
int wo_mesh_write_obj(char const* path, Wo_MeshVertex const* vertices, uint32_t n_vertices, Wo_MeshQuad const* quads,
                      Wo_MeshQuadIds const* ids_or_null, uint32_t n_quads);

/* Path-tracer kernel selection (results are identical; only speed differs).
 *   AUTO         union-only scenes of more than WOLOLO_LANES_MIN_PRIMS (256)
 *                primitives -> LANES; else scenes of up to WOLOLO_JIT_MAX_PRIMS
 *                (256) primitives -> JIT; else INTERPRETER.
 *   INTERPRETER  the postfix-program interpreter kernel.
 *   JIT          the scene-specialised kernel, compiled with hiprtc at scene
 *                upload, for scenes of up to WOLOLO_JIT_MAX_PRIMS primitives
 *                (else, or if compilation fails, the interpreter).
 *   LANES        per-lane BOUND traversal, for union-only scenes (others fall
 *                back to AUTO's choice).
 * Environment: WOLOLO_TRACER=auto|interpreter|jit|lanes sets the initial value.
 * Takes effect at the next render. */
typedef enum Wo_Tracer {
    WO_TRACER_AUTO = 0,
    WO_TRACER_INTERPRETER = 1,
    WO_TRACER_JIT = 2,
    WO_TRACER_LANES = 3,
} Wo_Tracer;
void wo_renderer_set_tracer(Wo_Renderer* r, Wo_Tracer tracer);
/* Compatibility form: 0 = INTERPRETER, anything else = AUTO. */
void wo_renderer_set_jit(Wo_Renderer* r, int mode);
/* Which path kernel the last render used: "jit", "lanes", "interpreter" or "none". */
char const* wo_renderer_trace_path(Wo_Renderer* r);
/* Scene edits do not stall draw_frame (on by default; WOLOLO_JIT_ASYNC=0 turns it
 * off): when the specialised kernel of the edited scene is in neither code-object
 * cache, draw_frame starts its hiprtc compile on a background host thread and
 * renders with the interpreter -- the same image bit for bit -- until the compile
 * has ended; the first draw_frame after that switches to it.  render_f32,
 * render_accumulate, render_rows_device, render_frame_device and count_work wait
 * for a compile in flight (batch renders get the specialised kernel) -- except
 * under WO_TRACER_AUTO for a general tree above 256 primitives (1-2 minutes of
 * hiprtc), which the lane tracer renders meanwhile in batch renders too.  The
 * nodes are added incrementally as in the reference (renderer.c:2232-2275). */
void wo_renderer_set_jit_async(Wo_Renderer* r, int on);
/* 1 while a background compile of the current scene's kernel is in flight. */
int wo_renderer_jit_pending(Wo_Renderer* r);
/* Compile, upload and load the current scene's kernels now, waiting for any
 * background compile (a benchmark's set-up: the timed frames then run the
 * kernel AUTO settles on).  Extends the reference's per-frame scene upload
 * (renderer.c:2085-2219 records it into every frame); 0, or -1 on failure. */
int wo_renderer_prepare(Wo_Renderer* r);

/* HIP source of the scene-specialised kernel for the current scene (NULL if
 * the scene has no primitives); release with wo_free(). */
char* wo_renderer_jit_source(Wo_Renderer* r);
/* Compile `src` with hiprtc for `arch` (e.g. "gfx950") without loading it --
 * needs no GPU.  Returns 0, or -1 with the compiler log in err. */
int wo_jit_compile_check(char const* src, char const* arch, char* err, size_t errlen);
/* Code object of the specialised kernel `src` for `arch`, as a render would get
 * it: from this process's cache, else the on-disk cache (WOLOLO_JIT_CACHE =
 * directory, "0" = off; default $XDG_CACHE_HOME/wololo/jit or
 * ~/.cache/wololo/jit; entries keyed by the SHA-256 of source, headers,
 * target, options and hiprtc version), else compiled with hiprtc and stored.
 * *origin: 0 process cache, 1 disk cache, 2 compiled; *seconds: time taken;
 * key_hex (65 bytes or NULL): the key.  Returns the object's size or -1 (err).
 * Needs no GPU. */
long long wo_jit_code_object(char const* src, char const* arch, int* origin, double* seconds, char* key_hex,
                             char* err, size_t errlen);
/* The specialised kernel's resources as its code object states them (its AMDHSA
 * kernel descriptor, as wo_renderer_kernel_info reports them): out[0] scratch bytes
 * per lane (the private segment), out[1] static LDS bytes per workgroup (the group
 * segment).  Compiles (or takes from the caches) like wo_jit_code_object.  Returns 0,
 * or -1 (err).  Needs no GPU. */
int wo_jit_code_resources(char const* src, char const* arch, uint32_t* out, char* err, size_t errlen);
/* Where the renderer's specialised kernel came from (origin as above; -1: the
 * renderer does not run one) and the seconds it took (compile or load). */
int wo_renderer_jit_info(Wo_Renderer* r, double* seconds);
/* The lane tracer's BVH (union-only scenes): out[0] internal nodes, out[1] its
 * depth in internal levels (= the per-lane LDS stack entries; at most 24),
 * out[2] top nodes staged in LDS, out[3] primitives tested on every query (no
 * box), out[4] the kernel form of the last path or ray launch (0-14 the lane tracer's
 * forms, 11-14 the resumable walk; wo_dev_impl.h PathKind).  `out` holds 5
 * entries.  Returns 0, or -1 when the renderer does not run the lane tracer
 * (neither its path kernel nor its last ray query). */
int wo_renderer_lanes_info(Wo_Renderer* r, uint32_t* out);
/* The path kernel of the last launch as the runtime loaded it: key_hex (65 bytes)
 * gets the specialised kernel's code-object key (SHA-256 of source, options and
 * toolchain) or "static:<kind>:<40 hex digits of the library kernels' source hash>"; out[0] = kind (as lanes_info's), out[1] = private
 * (scratch) bytes per lane, out[2] = VGPRs, out[3] = static LDS bytes.  Profile
 * sessions record it beside their counters.  0, or -1 before any path launch. */
int wo_renderer_kernel_info(Wo_Renderer* r, char* key_hex, uint32_t* out);
void wo_free(void* p);

size_t wo_renderer_node_count(Wo_Renderer* r);
char const* wo_renderer_name(Wo_Renderer* r);
/* HIP device ordinal the renderer runs on; -1 for a device-less renderer. */
int wo_renderer_device(Wo_Renderer* r);
char const* wo_renderer_last_error(void);
/* Empty this thread's last-error message (so a caller can tell a new failure). */
void wo_renderer_clear_error(void);

/* ---- library-level ---- */
/* sizeof(type) (field NULL) or offsetof(type, field) as this library was
 * compiled, for the value types of the C ABI (Wo_Vec3, Wo_Quaternion,
 * Wo_Node_Argument, Wo_RenderParams, WoRec, WoMaterial, WoCamera, WoFrame, Wo_Ray, Wo_RayHit,
 * Wo_RayCrossing, Wo_RaySpans, Wo_MassGrid, Wo_MassPlan, Wo_MassSums, Wo_MassProperties,
 * Wo_FeatureIds, Wo_DenoiseParams, Wo_MeshGrid, Wo_MeshVertex, Wo_MeshQuad, Wo_MeshQuadIds, Wo_MeshCounts,
 * Wo_Mesh);
 * (size_t)-1 for an unknown name.  Bindings check their mirrors with it. */
size_t wo_abi_layout(char const* type, char const* field);
/* Device self-check of the path tracer's fast correctly rounded square root
 * (which = 0) or reciprocal (1) against the IEEE expansions, over every float
 * bit pattern in [lo_bits, hi_bits] (on the current HIP device, synchronous).
 * 0 and the mismatch count / smallest mismatching pattern, or -1. */
int wo_fastmath_check(int which, uint32_t lo_bits, uint32_t hi_bits, unsigned long long* mismatches,
                      uint32_t* first_mismatch);
char const* wo_version(void);
/* Number of visible HIP devices (0 when none / no driver). */
int wo_hip_device_count(void);
/* Version of the HIP runtime this process uses (hipRuntimeGetVersion, e.g.
 * 70226015), or -1.  The scene-specialised kernels are compiled by the hiprtc of
 * the same installation: whichever libamdhip64.so.7 / libhiprtc.so.7 the process
 * loaded first (a PyTorch wheel bundles its own). */
int wo_hip_runtime_version(void);

#ifdef __cplusplus
}
#endif

#endif /* WOLOLO_RENDERER_RENDERER_EXT_H */
