/*
 * mass.c -- the host side of the mass-properties query (renderer_ext.h Wo_MassGrid):
 * the plan that host and kernel derive from a grid, and the finalisation of the
 * exact integer sums into volume, centroid and inertia.  Host only, no HIP:
 * tests/host/mass_main.c drives it under ASan + UBSan (make mass-asan).
 */
#include <math.h>
#include <string.h>

#include "wo_internal.h"

#define WO_MASS_PAD 0x1p-9f
_Static_assert(WO_MASS_PAD > WO_T_MIN, "a surface on the clip box's near face must be a crossing (t > WO_T_MIN)");
_Static_assert(sizeof(Wo_MassGrid) == 48 && sizeof(Wo_MassSums) == 192, "Wo_MassGrid is 48 bytes, Wo_MassSums 192");

static uint32_t mass_q(float t, float scale) {
    const float p = t * scale; /* exact: scale is a power of two and nothing under- or overflows for |k| <= 100 */
    return (uint32_t)rintf(p);
}

int wo_mass_grid_plan(Wo_MassGrid const* g, Wo_MassPlan* plan) {
    if (!g || !plan) {
        wo_set_error("mass grid: NULL grid or plan");
        return -1;
    }
    for (int a = 0; a < 3; ++a) {
        if (!isfinite(g->lo[a]) || !isfinite(g->hi[a])) {
            wo_set_error("mass grid: clip box is not finite on axis %d", a);
            return -1;
        }
        if (!(g->lo[a] < g->hi[a])) {
            wo_set_error("mass grid: clip box needs lo < hi on axis %d (%g, %g)", a, (double)g->lo[a], (double)g->hi[a]);
            return -1;
        }
    }
    if (g->axis > 2u) {
        wo_set_error("mass grid: axis %u (0, 1 or 2)", g->axis);
        return -1;
    }
    if (g->nu == 0u || g->nu > WO_MASS_MAX_CELLS || g->nv == 0u || g->nv > WO_MASS_MAX_CELLS) {
        wo_set_error("mass grid: %u x %u cells (1 .. %u each)", g->nu, g->nv, WO_MASS_MAX_CELLS);
        return -1;
    }
    if (g->v_count == 0u || g->v_begin >= g->nv || g->v_count > g->nv - g->v_begin) {
        wo_set_error("mass grid: rows [%u, %u + %u) are not rows of the %u", g->v_begin, g->v_begin, g->v_count, g->nv);
        return -1;
    }
    if (g->reserved != 0u) {
        wo_set_error("mass grid: reserved must be 0");
        return -1;
    }
    const uint32_t ax = g->axis, u = (ax + 1u) % 3u, v = (ax + 2u) % 3u;
    Wo_MassPlan p;
    memset(&p, 0, sizeof p);
    p.pad = WO_MASS_PAD;
    p.o_axis = g->lo[ax] - p.pad;
    const float extent = g->hi[ax] - g->lo[ax];
    p.t_max = p.pad + extent;
    const float eu = g->hi[u] - g->lo[u], ev = g->hi[v] - g->lo[v];
    p.u0 = g->lo[u];
    p.hu = eu / (float)(2u * g->nu);
    p.v0 = g->lo[v];
    p.hv = ev / (float)(2u * g->nv);
    if (!isfinite(p.o_axis) || !isfinite(p.t_max) || !isfinite(p.hu) || !isfinite(p.hv)) {
        wo_set_error("mass grid: the clip box's extent overflows fp32");
        return -1;
    }
    if (!(p.hu > 0.0f) || !(p.hv > 0.0f)) {
        wo_set_error("mass grid: a cell's width underflows fp32");
        return -1;
    }
    int e = 0;
    (void)frexpf(p.t_max, &e);
    p.k = 20 - e;
    if (p.k > 100 || p.k < -100) {
        wo_set_error("mass grid: extent %g along the rays is out of range (k = %d)", (double)p.t_max, p.k);
        return -1;
    }
    p.scale = ldexpf(1.0f, p.k);
    p.q0 = mass_q(p.pad, p.scale);
    p.q1 = mass_q(p.t_max, p.scale);
    *plan = p;
    return 0;
}

int wo_mass_properties_from_sums(Wo_MassGrid const* g, Wo_MassSums const* sums, Wo_MassProperties* out) {
    if (!sums || !out) {
        wo_set_error("mass properties: NULL sums or result");
        return -1;
    }
    Wo_MassPlan p;
    if (wo_mass_grid_plan(g, &p)) return -1;
    double S[10];
    for (int s = 0; s < 10; ++s) S[s] = (double)((unsigned __int128)sums->lo[s] + ((unsigned __int128)sums->hi[s] << 32));
    const uint32_t ax = g->axis, u = (ax + 1u) % 3u, v = (ax + 2u) % 3u;
    const double h = ldexp(1.0, -p.k), hu = (double)p.hu, hv = (double)p.hv;
    const double A = (2.0 * hu) * (2.0 * hv);
    memset(out, 0, sizeof *out);
    out->cell[0] = 2.0 * hu;
    out->cell[1] = 2.0 * hv;
    out->cell[2] = h;
    out->rays = sums->rays;
    out->crossings = sums->crossings;
    out->projected_area = (double)sums->rays_hit * A;
    if (S[0] == 0.0) {
        for (int a = 0; a < 3; ++a) out->centroid[a] = 0.5 * ((double)g->lo[a] + (double)g->hi[a]);
        return 0;
    }
    const double V = A * h * S[0];
    /* local means and second moments, in the order (u, v, t) */
    const double mean[3] = {hu * S[1] / S[0], hv * S[2] / S[0], 0.5 * h * S[3] / S[0]};
    double E[3][3];
    E[0][0] = A * h * (hu * hu * S[4] + hu * hu / 3.0 * S[0]);
    E[1][1] = A * h * (hv * hv * S[5] + hv * hv / 3.0 * S[0]);
    E[2][2] = A * h * h * h / 3.0 * S[6];
    E[0][1] = E[1][0] = A * h * hu * hv * S[7];
    E[0][2] = E[2][0] = A * h * h / 2.0 * hu * S[8];
    E[1][2] = E[2][1] = A * h * h / 2.0 * hv * S[9];
    double C[3][3], trace = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) C[a][b] = E[a][b] - V * mean[a] * mean[b];
    for (int a = 0; a < 3; ++a) trace += C[a][a];
    const uint32_t world[3] = {u, v, ax}; /* local axis -> x, y, z */
    out->volume = V;
    out->centroid[u] = (double)g->lo[u] + mean[0];
    out->centroid[v] = (double)g->lo[v] + mean[1];
    out->centroid[ax] = (double)p.o_axis + mean[2];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) out->inertia[world[a] * 3u + world[b]] = (a == b ? trace : 0.0) - C[a][b];
    return 0;
}
