/*
 * span_ref.c -- CPU reference of the ray span query (wo_renderer_trace_spans), TEST
 * INFRASTRUCTURE, built by tests/test_spans.py as a shared object with the oracle
 * Makefile's flags.
 *
 * It states no geometry of its own: leaf intervals (leaf_span), the primitive table
 * (scratch_init), event keys (make_key), their order (cmp_event) and the tree's value
 * (eval_tree) are the oracle's functions, and the collection below is trace_ray's
 * (oracle.c) line for line.  Where trace_ray returns at the first flip of the root,
 * this lists every flip up to t_max and sums the length inside, as renderer_ext.h
 * defines Wo_RaySpans.
 */
#include "../../oracle/oracle.c"

/* One ray: o, d, t_max.  Out: ts / los / afters[k] for the first min(count, max_out)
 * crossings (lo = ordinal << 12 | type << 11 | member, the key's low word; after = the
 * root's value behind the crossing), *inside0 the root at WO_T_MIN, *length as defined,
 * *n_events the events with t > WO_T_MIN over all primitives.  Returns the count of all
 * crossings in (WO_T_MIN, t_max]. */
static uint32_t span_ray(const WoRec* prog, uint32_t n, Scratch* s, const float o[3], const float d[3], float t_max,
                         uint32_t max_out, float* ts, uint32_t* los, uint32_t* afters, uint32_t* inside0,
                         float* length, uint32_t* n_events) {
    const float tmin = WO_T_MIN;
    uint32_t nev = 0;
    for (uint32_t k = 0; k < s->nprims; ++k) {
        float lo, hi;
        uint32_t mlo = 0, mhi = 0;
        leaf_span(&prog[s->prims[k].pc + 1u], o, d, &lo, &hi);
        for (uint32_t m = 1; m < s->prims[k].count; ++m) {
            float a, b;
            leaf_span(&prog[s->prims[k].pc + 1u + m], o, d, &a, &b);
            if (a > lo) {
                lo = a;
                mlo = m;
            }
            if (b < hi) {
                hi = b;
                mhi = m;
            }
        }
        s->inside[k] = 0;
        if (lo > hi) continue; /* empty */
        s->inside[k] = (lo <= tmin && hi > tmin) ? 1 : 0;
        if (lo > tmin) s->ev[nev++].key = make_key(lo, k, 0u, mlo);
        if (hi > tmin && hi < INFINITY) s->ev[nev++].key = make_key(hi, k, 1u, mhi);
    }
    *n_events = nev;
    qsort(s->ev, nev, sizeof(Event), cmp_event);
    int root = eval_tree(prog, n, s->inside, s->stack);
    *inside0 = (uint32_t)root;
    uint32_t count = 0;
    float len = 0.0f, t_in = tmin;
    for (uint32_t i = 0; i < nev; ++i) {
        union {
            uint32_t u;
            float f;
        } tb;
        tb.u = (uint32_t)(s->ev[i].key >> 32);
        if (tb.f > t_max) break;
        uint32_t lo32 = (uint32_t)s->ev[i].key;
        s->inside[lo32 >> 12] ^= 1u;
        int r = eval_tree(prog, n, s->inside, s->stack);
        if (r == root) continue;
        if (count < max_out) {
            ts[count] = tb.f;
            los[count] = lo32;
            afters[count] = (uint32_t)r;
        }
        ++count;
        if (r)
            t_in = tb.f;
        else
            len = len + (tb.f - t_in);
        root = r;
    }
    if (root && t_max > t_in) len = len + (t_max - t_in);
    *length = len;
    return count;
}

/* n rays as Wo_Ray rows (8 floats: origin, t_max, dir, reserved), all taken as valid.
 * Per ray i: counts[i], inside0[i], lengths[i], n_events[i], and its crossings at
 * ts / los / afters[i * max_out + k].  0, or -1 (out of memory). */
int span_ref(WoRec const* prog, uint32_t n_recs, float const* rays, uint32_t n, uint32_t max_out, uint32_t* counts,
             uint32_t* inside0, float* lengths, uint32_t* n_events, float* ts, uint32_t* los, uint32_t* afters) {
    Scratch s;
    if (scratch_init(&s, prog, n_recs)) {
        scratch_free(&s);
        return -1;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const float* r = rays + 8u * (size_t)i;
        const size_t at = (size_t)i * max_out;
        counts[i] = span_ray(prog, n_recs, &s, r, r + 4, r[3], max_out, ts + at, los + at, afters + at, &inside0[i],
                             &lengths[i], &n_events[i]);
    }
    scratch_free(&s);
    return 0;
}
