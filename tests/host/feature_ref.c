/*
 * feature_ref.c -- CPU reference of the first-hit feature buffers
 * (wo_renderer_render_features), TEST INFRASTRUCTURE, built by tests/feature_support.py
 * as a shared object with the oracle Makefile's flags.
 *
 * It states no arithmetic of its own beyond the order renderer_ext.h gives: the RNG
 * (oracle_pcg_hash, rng_float), the lens (sqrt_pt, sincos_turn), normalize3, the segment
 * query (trace_ray), sky_color and the 32.32 accumulation (quantize_radiance,
 * mean_radiance) are the oracle's functions, and the camera ray is shade_pixel's
 * (oracle.c) line for line.  tests/test_features.py pins the rays and the RNG to the
 * oracle's own frames independently.
 */
#include "../../oracle/oracle.c"

/* shade_pixel's camera ray of sample smp of pixel (x, y); centre: its NORMALS sample */
static void feature_ray(const WoFrame* fr, uint32_t x, uint32_t y, uint32_t smp, int centre, float o[3], float d[3]) {
    const WoCamera* cam = &fr->cam;
    const uint32_t W = fr->width, H = fr->height;
    const uint32_t pixel = y * W + x;
    uint32_t rng = oracle_pcg_hash(pixel ^ oracle_pcg_hash((fr->sample_offset + smp) ^ oracle_pcg_hash(fr->seed)));
    float u, v;
    if (centre) {
        u = ((float)x + 0.5f) * fr->inv_width;
        v = ((float)(H - 1u - y) + 0.5f) * fr->inv_height;
    } else {
        float jx = rng_float(&rng);
        float jy = rng_float(&rng);
        u = ((float)x + jx) * fr->inv_width;
        v = ((float)(H - 1u - y) + jy) * fr->inv_height;
    }
    float off[3] = {0.0f, 0.0f, 0.0f};
    if (cam->lens_radius > 0.0f && !centre) {
        float rad = sqrt_pt(rng_float(&rng));
        float s, c;
        sincos_turn(rng_float(&rng), &s, &c);
        float px = rad * c, py = rad * s;
        float rx = cam->lens_radius * px, ry = cam->lens_radius * py;
        for (int i = 0; i < 3; ++i) off[i] = cam->u[i] * rx + cam->v[i] * ry;
    }
    for (int i = 0; i < 3; ++i) {
        o[i] = cam->origin[i] + off[i];
        d[i] = ((cam->lower_left[i] + u * cam->horizontal[i]) + v * cam->vertical[i]) - cam->origin[i] - off[i];
    }
    normalize3(d);
}

/* npix pixels (xs, ys) of frame fr (width, height, spp, seed, sample_offset, inv_*, cam).
 * Per pixel i: albedo[4 i ..] and normal[4 i ..] as the planes define them, ids[4 i ..] =
 * node, leaf, material, flags; and for diagnostics hits[i] and the raw sums[7 i ..] =
 * albedo rgb, normal xyz, t.  `nodes`: per record its source node.  0, or -1 (out of memory). */
int feature_ref(WoRec const* prog, uint32_t n_recs, WoMaterial const* mats, uint32_t n_mats, uint32_t const* nodes,
                WoFrame const* fr, uint32_t const* xs, uint32_t const* ys, uint32_t npix, float* albedo,
                float* normal, uint32_t* ids, uint32_t* hits, int64_t* sums) {
    Scratch s;
    if (scratch_init(&s, prog, n_recs)) {
        scratch_free(&s);
        return -1;
    }
    const uint32_t spp = fr->spp;
    for (uint32_t i = 0; i < npix; ++i) {
        int64_t sa[3] = {0, 0, 0}, sn[3] = {0, 0, 0}, st = 0;
        uint32_t nh = 0;
        float o[3], d[3];
        OHit h;
        for (uint32_t smp = 0; smp < spp; ++smp) {
            feature_ray(fr, xs[i], ys[i], smp, 0, o, d);
            float a[3];
            if (trace_ray(prog, n_recs, &s, o, d, &h)) {
                const WoRec* L = &prog[s.prims[h.ord].pc + 1u + h.member];
                float P[3] = {o[0] + h.t * d[0], o[1] + h.t * d[1], o[2] + h.t * d[2]};
                for (int k = 0; k < 3; ++k) {
                    float nl = L->op == WO_LEAF_SPHERE ? (P[k] - L->f[k]) * L->f[4] : L->f[k];
                    float N = h.type == 0u ? nl : -nl;
                    float ns = h.root_after != 0u ? N : -N;
                    sn[k] += quantize_radiance(ns);
                }
                const WoMaterial* m = &mats[L->u0 < n_mats ? L->u0 : 0u];
                const int opaque = m->kind == WO_MAT_LAMBERTIAN || m->kind == WO_MAT_METAL;
                for (int k = 0; k < 3; ++k) a[k] = opaque ? m->albedo[k] : 1.0f;
                st += quantize_radiance(h.t);
                ++nh;
            } else {
                sky_color(d, a);
            }
            for (int k = 0; k < 3; ++k) sa[k] += quantize_radiance(a[k]);
        }
        for (int k = 0; k < 3; ++k) {
            albedo[4u * (size_t)i + k] = mean_radiance(sa[k], spp);
            normal[4u * (size_t)i + k] = mean_radiance(sn[k], spp);
            sums[7u * (size_t)i + k] = sa[k];
            sums[7u * (size_t)i + 3 + k] = sn[k];
        }
        sums[7u * (size_t)i + 6] = st;
        hits[i] = nh;
        albedo[4u * (size_t)i + 3] = (float)((double)nh / (double)spp);
        normal[4u * (size_t)i + 3] = nh ? mean_radiance(st, nh) : INFINITY;
        /* the pixel-centre ray */
        uint32_t* id = ids + 4u * (size_t)i;
        feature_ray(fr, xs[i], ys[i], 0u, 1, o, d);
        if (trace_ray(prog, n_recs, &s, o, d, &h)) {
            const uint32_t leaf = s.prims[h.ord].pc + 1u + h.member;
            id[0] = nodes[leaf];
            id[1] = leaf;
            id[2] = prog[leaf].u0 < n_mats ? prog[leaf].u0 : 0u;
            id[3] = 1u | (h.type ? 2u : 0u) | (h.root_after ? 4u : 0u); /* WO_RAY_HIT | _EXIT | _ENTERS */
        } else {
            id[0] = id[1] = id[2] = 0xFFFFFFFFu;
            id[3] = 0u;
        }
    }
    scratch_free(&s);
    return 0;
}
