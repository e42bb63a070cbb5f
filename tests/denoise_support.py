"""Shared by tests/test_denoise.py and tests/test_gpu_denoise.py (test helper, no fixture): a numpy
float32 restatement of the a-trous denoiser as include/wololo/renderer/renderer_ext.h states it
(written from that text, not from csrc/denoise.c), and a seeded synthetic input that exercises
every term.  One array operation per scalar operation of the specification: numpy rounds each to
float32 and fuses nothing, and np.float32(1) / x is the correctly rounded reciprocal."""
import numpy as np

from csgrenderer_amd import wololo as wl

F = np.float32
IDS_DT = np.dtype(wl.FEATURE_IDS_FIELDS)
SENTINEL = 0xA5A5A5A5
H_TAPS = (F(0.375), F(0.25), F(0.0625))
INF = F(np.inf)


def clampf(v, lo, hi):
    t = np.where(v > lo, v, lo)
    return np.where(t < hi, t, hi)


def edge(d2, k):
    x = F(1) - d2 * k
    m = np.where(x > 0, x, F(0))
    return m * m


def dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _shift(a, dx, dy, fill=0):
    """b[y, x] = a[y + dy, x + dx] where that is in the frame (else `fill`), and the in-frame mask."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    m = np.zeros((h, w), dtype=bool)
    x0, x1 = max(0, -dx), min(w, w - dx)
    y0, y1 = max(0, -dy), min(h, h - dy)
    if x0 < x1 and y0 < y1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        m[y0:y1, x0:x1] = True
    return b, m


class Shares:
    """Per term, the off-centre in-frame taps whose E is 0, strictly between 0 and 1, and 1."""

    def __init__(self):
        self.n = {t: np.zeros(3, dtype=np.int64) for t in ("color", "normal", "depth")}

    def add(self, term, e, mask):
        v = e[mask]
        self.n[term] += (int((v == 0).sum()), int(((v > 0) & (v < 1)).sum()), int((v == 1).sum()))

    def share(self, term):
        """(zero, partial, one) as fractions of the term's taps; None if it saw none."""
        tot = int(self.n[term].sum())
        return None if tot == 0 else tuple(float(c) / tot for c in self.n[term])


def reference(dp, color, albedo=None, normal=None, ids=None):
    """(out (H, W, 4) float32, Shares) of the filter with Wo_DenoiseParams dp."""
    color = np.asarray(color, dtype=np.float32)
    h, w = color.shape[:2]
    k_color, k_normal, k_depth = F(dp.k_color), F(dp.k_normal), F(dp.k_depth)
    demod = bool(dp.flags & wl.DENOISE_DEMODULATE)
    stop = bool(dp.flags & wl.DENOISE_STOP_AT_NODES)
    shares = Shares()
    with np.errstate(all="ignore"):
        if demod:
            amod = clampf(np.asarray(albedo, dtype=np.float32)[..., :3], F(2.0 ** -7), F(2.0 ** 20))
            c = color[..., :3] * (F(1) / amod)
        else:
            c = color[..., :3].copy()
        if k_normal > 0 or k_depth > 0:
            nrm = np.asarray(normal, dtype=np.float32)
            n3, z = nrm[..., :3], nrm[..., 3]
            fin = z < INF
            rz = F(1) / clampf(z, F(2.0 ** -20), F(2.0 ** 20))
        if stop:
            ids = np.asarray(ids)
            node = ids["node"] if ids.dtype == IDS_DT else ids.view(np.uint32).reshape(h, w, 4)[..., 0]
        for i in range(int(dp.levels)):
            s = 1 << i
            kc = k_color * F(1 << (2 * i))
            total = np.zeros((h, w, 3), dtype=np.float32)
            wsum = np.zeros((h, w), dtype=np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    hh = H_TAPS[abs(dx)] * H_TAPS[abs(dy)]
                    cq, inframe = _shift(c, dx * s, dy * s)
                    if dx == 0 and dy == 0:
                        wt = np.full((h, w), hh, dtype=np.float32)
                    else:
                        e = np.ones((h, w), dtype=np.float32)
                        if k_color > 0:
                            t = edge(dist2(cq, c), kc)
                            shares.add("color", t, inframe)
                            e = e * t
                        if k_normal > 0:
                            nq, _ = _shift(n3, dx * s, dy * s)
                            t = edge(dist2(nq, n3), k_normal)
                            shares.add("normal", t, inframe)
                            e = e * t
                        if k_depth > 0:
                            zq, _ = _shift(z, dx * s, dy * s)
                            finq, _ = _shift(fin, dx * s, dy * s, fill=False)
                            rel = (zq - z) * rz
                            t = edge(rel * rel, k_depth)
                            t = np.where(fin & finq, t, np.where(fin != finq, F(0), F(1)))
                            shares.add("depth", t, inframe)
                            e = np.where(fin & finq, e * t, np.where(fin != finq, F(0), e))
                        if stop:
                            nodeq, _ = _shift(node, dx * s, dy * s)
                            e = np.where(nodeq != node, F(0), e)
                        wt = hh * e
                    take = inframe & (wt > 0)
                    total = np.where(take[..., None], total + wt[..., None] * cq, total)
                    wsum = np.where(take, wsum + wt, wsum)
            assert (wsum >= F(9.0 / 64.0)).all()
            c = total * (F(1) / wsum)[..., None]
        out = np.empty((h, w, 4), dtype=np.float32)
        out[..., :3] = c * amod if demod else c
    out.view(np.uint32)[..., 3] = color.view(np.uint32)[..., 3]
    return out, shares


def synthetic(w, h, seed=1):
    """A seeded w x h input of 9 x 7-pixel blocks: dict of color, albedo, normal (h, w, 4) float32, ids
    (h, w) IDS_DT, and the special pixels `nan` and `inf` ((x, y) or None).  Per block a node id, a
    unit normal (plus per-pixel noise of sigma 0.1), a depth in [1, 10] (+-3 % per pixel) and an albedo
    in [0, 1]; one block's albedo is exactly 0; a rectangle of sky has normal 0 and depth +inf; the
    colour is albedo * (0.5 + U[0, 1)); one pixel has a NaN channel and one a +inf channel."""
    rng = np.random.default_rng(seed)
    bw, bh = (w + 8) // 9, (h + 6) // 7
    by, bx = np.arange(h)[:, None] // 7, np.arange(w)[None, :] // 9
    block = by * bw + bx                                   # (h, w)
    nb = bw * bh
    nodes = rng.permutation(nb).astype(np.uint32) + 3
    bn = rng.normal(size=(nb, 3))
    bn /= np.linalg.norm(bn, axis=1, keepdims=True)
    bdepth = rng.uniform(1.0, 10.0, size=nb)
    balbedo = rng.uniform(0.0, 1.0, size=(nb, 3))
    if nb > 1:
        balbedo[nb // 2] = 0.0
    normal = np.zeros((h, w, 4), dtype=np.float32)
    normal[..., :3] = (bn[block] + rng.normal(scale=0.1, size=(h, w, 3))).astype(np.float32)
    normal[..., 3] = (bdepth[block] * (1.0 + rng.uniform(-0.03, 0.03, size=(h, w)))).astype(np.float32)
    albedo = np.zeros((h, w, 4), dtype=np.float32)
    albedo[..., :3] = balbedo[block].astype(np.float32)
    albedo[..., 3] = 1.0
    ids = np.zeros((h, w), dtype=IDS_DT)
    ids["node"] = nodes[block]
    ids["leaf"] = nodes[block] + 100
    ids["material"] = block % 5
    ids["flags"] = wl.RAY_HIT | wl.RAY_ENTERS
    if w >= 12 and h >= 10:  # the sky: across block borders, off the frame's corner
        sy, sx = slice(h // 2, h // 2 + max(3, h // 4)), slice(w // 3, w // 3 + max(4, w // 3))
        normal[sy, sx] = (0.0, 0.0, 0.0, np.inf)
        albedo[sy, sx, :3] = rng.uniform(0.3, 1.0, size=3).astype(np.float32)
        albedo[sy, sx, 3] = 0.0
        ids[sy, sx] = (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0)
    color = np.zeros((h, w, 4), dtype=np.float32)
    color[..., :3] = albedo[..., :3] * (0.5 + rng.uniform(0.0, 1.0, size=(h, w, 3))).astype(np.float32)
    color[..., 3] = rng.uniform(0.0, 1.0, size=(h, w)).astype(np.float32)  # an alpha that is not constant
    nan = inf = None
    if w * h > 1:
        nan, inf = (w // 3, h // 3), ((2 * w) // 3, (2 * h) // 3)
        color[nan[1], nan[0], 1] = np.nan
        color[inf[1], inf[0], 0] = np.inf
    out = {"color": color, "albedo": albedo, "normal": normal, "ids": ids, "nan": nan, "inf": inf}
    for a in (color, albedo, normal, ids):
        a.setflags(write=False)
    return out


_INPUTS = {}


def synthetic_shared(w, h, seed=1):
    """synthetic(), made once per size and shared (read-only)."""
    key = (w, h, seed)
    if key not in _INPUTS:
        _INPUTS[key] = synthetic(w, h, seed)
    return _INPUTS[key]


# what the tests run: (name, parameters, which optional planes are passed)
def cases():
    """[(name, dict of Wo_DenoiseParams fields without levels, planes passed (albedo, normal, ids))]: each
    term alone, all together, each flag on and off, NULL optional planes."""
    D, S = wl.DENOISE_DEMODULATE, wl.DENOISE_STOP_AT_NODES
    return [
        ("color", dict(flags=0, k_color=1.0, k_normal=0.0, k_depth=0.0), (False, False, False)),
        ("normal", dict(flags=0, k_color=0.0, k_normal=4.0, k_depth=0.0), (False, True, False)),
        ("depth", dict(flags=0, k_color=0.0, k_normal=0.0, k_depth=100.0), (True, True, True)),
        ("all", dict(flags=D, k_color=1.0, k_normal=4.0, k_depth=100.0), (True, True, False)),
        ("all+stop", dict(flags=D | S, k_color=1.0, k_normal=4.0, k_depth=100.0), (True, True, True)),
        ("stop", dict(flags=S, k_color=0.0, k_normal=0.0, k_depth=0.0), (False, False, True)),
        ("demod", dict(flags=D, k_color=0.0, k_normal=0.0, k_depth=0.0), (True, False, False)),
        ("none", dict(flags=0, k_color=0.0, k_normal=0.0, k_depth=0.0), (False, False, False)),
    ]


def case_params(fields, levels):
    return wl.denoise_params(levels=levels, **fields)


def case_planes(inp, passed):
    """(albedo, normal, ids) of the input, None where the case passes NULL."""
    return tuple(inp[k] if on else None for k, on in zip(("albedo", "normal", "ids"), passed))


_REFS = {}


def reference_shared(name, fields, passed, levels, w, h):
    """reference() of a case on the shared synthetic input, made once and shared (read-only)."""
    key = (name, levels, w, h)
    if key not in _REFS:
        inp = synthetic_shared(w, h)
        out, shares = reference(case_params(fields, levels), inp["color"], *case_planes(inp, passed))
        out.setflags(write=False)
        _REFS[key] = (out, shares)
    return _REFS[key]


def check_shares(shares, dp, what):
    """Every enabled term has at least 5 % of its taps at zero and at least 5 % partial: a condition
    on the reference alone, which catches an input that has stopped exercising a term."""
    for term, k in (("color", dp.k_color), ("normal", dp.k_normal), ("depth", dp.k_depth)):
        if k > 0:
            zero, partial, _ = shares.share(term)
            assert zero >= 0.05 and partial >= 0.05, (what, term, zero, partial)


def same_bits(got, exp, what):
    g = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32)
    e = np.ascontiguousarray(exp, dtype=np.float32).view(np.uint32)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    bad = (g != e).any(axis=-1)
    if bad.any():
        first = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: not bit-exact at {int(bad.sum())} of {bad.size} pixels, first (y, x) = {first}: "
                             f"got {got[first]} ({g[first]}), expected {exp[first]} ({e[first]})")
