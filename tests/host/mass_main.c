/* Stand-alone driver of csrc/mass.c (make -C csgrenderer_amd/csrc mass-asan builds it with
 * ASan + UBSan): wo_mass_grid_plan and wo_mass_properties_from_sums over a table of
 * grids, bad ones included, and hand-made sums whose properties are known in closed form.
 * Exit status 0 and "mass driver: ok" when every check holds. */
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "wololo/renderer/renderer_ext.h"

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

static Wo_MassGrid grid(float x0, float y0, float z0, float x1, float y1, float z1, uint32_t axis, uint32_t nu,
                        uint32_t nv) {
    Wo_MassGrid g;
    memset(&g, 0, sizeof g);
    g.lo[0] = x0, g.lo[1] = y0, g.lo[2] = z0;
    g.hi[0] = x1, g.hi[1] = y1, g.hi[2] = z1;
    g.axis = axis, g.nu = nu, g.nv = nv, g.v_begin = 0, g.v_count = nv;
    return g;
}

static int close_to(double got, double want, double scale) { return fabs(got - want) <= 1e-12 * scale; }

/* the sums of a solid that fills the clip box: every ray is the span [q0, q1] */
static Wo_MassSums full_box_sums(Wo_MassGrid const* g, Wo_MassPlan const* p) {
    Wo_MassSums s;
    memset(&s, 0, sizeof s);
    const uint64_t a = p->q0, b = p->q1;
    const uint64_t m0 = b - a, m1 = b * b - a * a, m2 = b * b * b - a * a * a;
    for (uint32_t j = g->v_begin; j < g->v_begin + g->v_count; ++j)
        for (uint32_t i = 0; i < g->nu; ++i) {
            const uint64_t i2 = 2u * i + 1u, j2 = 2u * j + 1u;
            const uint64_t term[10] = {m0, m0 * i2, m0 * j2, m1, m0 * i2 * i2, m0 * j2 * j2, m2, m0 * i2 * j2,
                                       m1 * i2, m1 * j2};
            for (int k = 0; k < 10; ++k) {
                s.lo[k] += term[k] & 0xFFFFFFFFull;
                s.hi[k] += term[k] >> 32;
            }
            s.rays += 1, s.rays_hit += 1;
        }
    return s;
}

static void good_grids(void) {
    /* dyadic box 4 x 2 x 8 at (-2, -1, -4): every plan value is known exactly */
    for (uint32_t axis = 0; axis < 3; ++axis) {
        Wo_MassGrid g = grid(-2.0f, -1.0f, -4.0f, 2.0f, 1.0f, 4.0f, axis, 16, 8);
        Wo_MassPlan p;
        CHECK(wo_mass_grid_plan(&g, &p) == 0, "axis %u: %s", axis, g_error);
        const float ext[3] = {4.0f, 2.0f, 8.0f};
        const uint32_t u = (axis + 1u) % 3u, v = (axis + 2u) % 3u;
        int e = 0;
        (void)frexpf(0x1p-9f + ext[axis], &e);
        CHECK(p.pad == 0x1p-9f && p.o_axis == g.lo[axis] - 0x1p-9f && p.t_max == 0x1p-9f + ext[axis], "axis %u plan", axis);
        CHECK(p.k == 20 - e && p.scale == ldexpf(1.0f, p.k), "axis %u: k %d scale %g", axis, p.k, (double)p.scale);
        CHECK(p.q0 == (uint32_t)ldexp(1.0, p.k - 9) && p.q1 == p.q0 + (uint32_t)ldexp((double)ext[axis], p.k),
              "axis %u: q0 %u q1 %u", axis, p.q0, p.q1);
        CHECK(p.q1 <= (1u << 20), "axis %u: q1 %u", axis, p.q1);
        CHECK(p.u0 == g.lo[u] && p.hu == ext[u] / 32.0f && p.v0 == g.lo[v] && p.hv == ext[v] / 16.0f, "axis %u cells", axis);

        /* the solid fills the box: its volume, centre and inertia, exactly representable */
        Wo_MassSums s = full_box_sums(&g, &p);
        Wo_MassProperties m;
        CHECK(wo_mass_properties_from_sums(&g, &s, &m) == 0, "axis %u: %s", axis, g_error);
        const double V = 64.0;
        CHECK(close_to(m.volume, V, V), "axis %u volume %.17g", axis, m.volume);
        for (int a = 0; a < 3; ++a) CHECK(close_to(m.centroid[a], 0.0, 8.0), "axis %u centroid[%d] %.17g", axis, a, m.centroid[a]);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                const int o1 = (a + 1) % 3, o2 = (a + 2) % 3;
                const double want = a == b ? V / 12.0 * ((double)ext[o1] * ext[o1] + (double)ext[o2] * ext[o2]) : 0.0;
                CHECK(close_to(m.inertia[3 * a + b], want, V * 64.0), "axis %u inertia[%d][%d] %.17g want %.17g", axis, a, b,
                      m.inertia[3 * a + b], want);
            }
        CHECK(close_to(m.projected_area, (double)ext[u] * ext[v], 64.0), "axis %u area %.17g", axis, m.projected_area);
        CHECK(m.cell[0] == 2.0 * p.hu && m.cell[1] == 2.0 * p.hv && m.cell[2] == ldexp(1.0, -p.k), "axis %u cell", axis);
        CHECK(m.rays == 128 && m.crossings == 0, "axis %u counters", axis);

        /* no solid at all */
        memset(&s, 0, sizeof s);
        s.rays = 128;
        CHECK(wo_mass_properties_from_sums(&g, &s, &m) == 0, "axis %u: %s", axis, g_error);
        CHECK(m.volume == 0.0 && m.centroid[0] == 0.0 && m.centroid[1] == 0.0 && m.centroid[2] == 0.0, "axis %u empty", axis);
        for (int a = 0; a < 9; ++a) CHECK(m.inertia[a] == 0.0, "axis %u empty inertia[%d]", axis, a);
    }
    /* the largest grid's last rows with the largest limbs, huge and tiny extents, negative k */
    {
        Wo_MassGrid g = grid(0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f, 2, 32768, 32768);
        g.v_begin = 32768 - 2, g.v_count = 2;
        Wo_MassPlan p;
        CHECK(wo_mass_grid_plan(&g, &p) == 0, "largest grid: %s", g_error);
        Wo_MassSums s = full_box_sums(&g, &p);
        Wo_MassProperties m;
        CHECK(wo_mass_properties_from_sums(&g, &s, &m) == 0, "largest grid: %s", g_error);
        CHECK(close_to(m.volume, 2.0 / 32768.0, 1.0) && m.rays == 65536, "largest grid volume %.17g", m.volume);
    }
    {
        Wo_MassGrid g = grid(-1e30f, -1e-30f, -3.0f, 1e30f, 1e-30f, 5.0f, 0, 3, 5);
        Wo_MassPlan p;
        CHECK(wo_mass_grid_plan(&g, &p) == 0 && p.k == -81 && p.q0 == 0 && p.q1 > (1u << 19) && p.q1 <= (1u << 20),
              "huge extent: %s k %d q1 %u", g_error, p.k, p.q1);
        g.axis = 1;
        CHECK(wo_mass_grid_plan(&g, &p) == 0 && p.k == 28 && p.q0 == (1u << 19) && p.q1 == (1u << 19),
              "tiny extent: %s k %d q0 %u q1 %u", g_error, p.k, p.q0, p.q1);
    }
}

static void bad_grids(void) {
    const Wo_MassGrid ok = grid(-1.0f, -1.0f, -1.0f, 1.0f, 1.0f, 1.0f, 0, 4, 4);
    Wo_MassGrid bad[16];
    int n = 0;
    for (int i = 0; i < 16; ++i) bad[i] = ok;
    bad[n++].lo[0] = NAN;
    bad[n++].hi[2] = INFINITY;
    bad[n++].lo[1] = -INFINITY;
    bad[n++].lo[1] = 1.0f;  /* lo == hi */
    bad[n++].hi[2] = -2.0f; /* lo > hi */
    bad[n++].axis = 3;
    bad[n++].nu = 0;
    bad[n++].nv = 0;
    bad[n++].nu = 32769;
    bad[n++].nv = 32769;
    bad[n++].v_count = 0;
    bad[n++].v_begin = 4;
    bad[n].v_begin = 2, bad[n++].v_count = 3;
    bad[n].v_begin = 1, bad[n++].v_count = 0xFFFFFFFFu; /* v_begin + v_count wraps */
    bad[n++].reserved = 1;
    bad[n].lo[0] = -3e38f, bad[n++].hi[0] = 3e38f; /* the extent overflows */
    Wo_MassPlan p;
    Wo_MassSums s;
    Wo_MassProperties m;
    memset(&s, 0, sizeof s);
    CHECK(wo_mass_grid_plan(&ok, &p) == 0, "%s", g_error);
    for (int i = 0; i < n; ++i) {
        g_error[0] = 0;
        CHECK(wo_mass_grid_plan(&bad[i], &p) == -1 && g_error[0], "bad grid %d was accepted", i);
        g_error[0] = 0;
        CHECK(wo_mass_properties_from_sums(&bad[i], &s, &m) == -1 && g_error[0], "bad grid %d was finalised", i);
    }
    /* an extent along the rays beyond |k| <= 100 */
    Wo_MassGrid far = grid(-1e37f, -1.0f, -1.0f, 1e37f, 1.0f, 1.0f, 0, 4, 4);
    CHECK(wo_mass_grid_plan(&far, &p) == -1, "k < -100 was accepted");
    far.axis = 1; /* the same box along y is fine */
    CHECK(wo_mass_grid_plan(&far, &p) == 0, "%s", g_error);
    CHECK(wo_mass_grid_plan(NULL, &p) == -1 && wo_mass_grid_plan(&ok, NULL) == -1, "NULL was accepted");
    CHECK(wo_mass_properties_from_sums(&ok, NULL, &m) == -1 && wo_mass_properties_from_sums(&ok, &s, NULL) == -1,
          "NULL was accepted");
}

int main(void) {
    good_grids();
    bad_grids();
    if (g_failed) {
        printf("mass driver: %d checks failed\n", g_failed);
        return 1;
    }
    printf("mass driver: ok\n");
    return 0;
}
