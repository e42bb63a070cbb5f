"""A float64 Monte-Carlo path tracer written from DESIGN.md section 3.1 (test helper).

It restates the shading the CPU oracle and the kernels implement -- camera, pixel jitter,
lens, Lambertian / metal / dielectric scattering, sky, the depth limit, the mean over spp --
in plain numpy, vectorised over paths, and shares no code, no compiled program and no random
stream with either: it reads the scene as `recorder.Recorder` recorded it (node graph, leaf
materials, camera tuple), finds hits by classifying points of the recorded graph, and draws
from its own numpy Generator.  Only expectations can be compared with it.

`mutate=` switches exactly one deliberate error on (MUTANTS); tests use the mutants to show
that the comparison would notice each of them.  They exist here only.
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np

T_MIN = 1.0e-3  # the hit is the first change of membership at t > 1e-3
SKY_HORIZON = np.array([0.5, 0.7, 1.0])
TIE = 1.0e-9  # roots closer than this (relative beyond t = 1) are one surface crossing

MUTANTS = ("lambert_uniform", "fuzz_ball", "metal_no_absorb", "schlick_pow4", "schlick_cos_transmitted",
           "ior_swapped", "no_tir", "lens_r_linear", "no_jitter", "row_flip", "sky_unnormalised",
           "depth_plus_one", "limit_returns_sky")

LAMBERTIAN, METAL, DIELECTRIC = 0, 1, 2


def sky(dy):
    """lerp(white, (0.5, 0.7, 1.0), (d.y + 1) / 2) for an array of d.y -> (..., 3)."""
    t = 0.5 * (np.asarray(dy, dtype=np.float64) + 1.0)
    return (1.0 - t)[..., None] + t[..., None] * SKY_HORIZON


def schlick(cosine, ior, power=5):
    r0 = ((1.0 - ior) / (1.0 + ior)) ** 2
    return r0 + (1.0 - r0) * (1.0 - cosine) ** power


class Camera:
    """The RTIOW look-at camera in double precision; row 0 is the top of the frame."""

    def __init__(self, cam, W, H):
        look_from, look_at, vup, vfov, aperture, focus = cam
        self.W, self.H = W, H
        self.origin = np.array(look_from, dtype=np.float64)
        w = self.origin - np.array(look_at, dtype=np.float64)
        w /= np.linalg.norm(w)
        u = np.cross(np.array(vup, dtype=np.float64), w)
        u /= np.linalg.norm(u)
        v = np.cross(w, u)
        vh = 2.0 * math.tan(math.radians(vfov) / 2.0)
        vw = vh * W / H
        self.u, self.v = u, v
        self.horizontal = focus * vw * u
        self.vertical = focus * vh * v
        self.lower_left = self.origin - self.horizontal / 2 - self.vertical / 2 - focus * w
        self.lens_radius = aperture / 2.0

    def rays(self, px, py, jx, jy, lens=None, row_flip=False):
        """Rays through pixel (px, py) at the in-pixel position (jx, jy) in [0, 1)^2, from the
        lens point `lens` (n, 2) on the unit disc.  Returns (origins, unit directions)."""
        s = (px + jx) / self.W
        t = ((py + jy) if row_flip else (self.H - 1 - py + jy)) / self.H
        o = np.broadcast_to(self.origin, (len(s), 3))
        if lens is not None and self.lens_radius > 0.0:
            o = o + self.lens_radius * (lens[:, :1] * self.u + lens[:, 1:] * self.v)
        d = self.lower_left + s[:, None] * self.horizontal + t[:, None] * self.vertical - o
        return o, d / np.linalg.norm(d, axis=1, keepdims=True)


class Scene:
    """The recorded graph flattened to world-space leaf instances and one boolean expression
    per root (an operand used twice gives two instances)."""

    def __init__(self, rec):
        self.kind, self.vec, self.sc, mats = [], [], [], []
        self.roots = [self._walk(rec, i, np.eye(3), np.zeros(3), mats)
                      for i in range(len(rec.nodes)) if i not in rec.nonroot]
        self.kind = np.array(self.kind)
        self.vec = np.array(self.vec, dtype=np.float64).reshape(-1, 3)
        self.sc = np.array(self.sc, dtype=np.float64)
        self.cam = rec.cam
        n = len(mats)
        self.mkind = np.zeros(n, dtype=np.int64)
        self.albedo = np.ones((n, 3))
        self.fuzz = np.zeros(n)
        self.ior = np.ones(n)
        for j, m in enumerate(mats):
            m = rec.mats[m]
            self.mkind[j] = {"lambertian": LAMBERTIAN, "metal": METAL, "dielectric": DIELECTRIC}[m[0]]
            if m[0] == "dielectric":
                self.ior[j] = m[1]
            else:
                self.albedo[j] = m[1]
                if m[0] == "metal":
                    self.fuzz[j] = min(max(m[2], 0.0), 1.0)

    def _walk(self, rec, node, M, c, mats):
        # a point p of this node's frame sits at M p + c in the world
        nd = rec.nodes[node]
        if nd[0] in "sh":
            if nd[0] == "s":  # |x - c| <= r
                self.kind.append(0)
                self.vec.append(c.copy())
                self.sc.append(abs(nd[1]))
            else:  # n.x <= n.c
                n = M @ (nd[1] / np.linalg.norm(nd[1]))
                self.kind.append(1)
                self.vec.append(n)
                self.sc.append(float(n @ c))
            mats.append(rec.leaf_mat.get(node, 0))
            return len(self.kind) - 1
        kids = []
        for a in nd[1:]:
            R, off = rec.placement(a)
            kids.append(self._walk(rec, a.node, M @ R, c + M @ off, mats))
        return (nd[0], kids[0], kids[1])

    def _eval(self, e, leaf_in):
        if not isinstance(e, tuple):
            return leaf_in[e]
        a, b = self._eval(e[1], leaf_in), self._eval(e[2], leaf_in)
        return a | b if e[0] == "u" else a & b if e[0] == "i" else a & ~b

    def leaf_membership(self, P):
        out = []
        for k, v, s in zip(self.kind, self.vec, self.sc):
            if k == 0:
                q = P - v
                out.append(np.einsum("ij,ij->i", q, q) <= s * s)
            else:
                out.append(P @ v <= s)
        return out

    def member(self, leaf_in, n):
        out = np.zeros(n, dtype=bool)
        for e in self.roots:
            out |= self._eval(e, leaf_in)
        return out

    def inside(self, P):
        return self.member(self.leaf_membership(P), len(P))

    def trace(self, o, d):
        """First root of a leaf surface beyond T_MIN at which the scene's membership flips.
        Returns (hit, t, N facing the ray, front, leaf)."""
        n, L = len(o), len(self.kind)
        T = np.full((n, 2 * L), np.inf)
        for j in range(L):
            if self.kind[j] == 0:
                oc = o - self.vec[j]
                b = np.einsum("ij,ij->i", oc, d)
                disc = b * b - (np.einsum("ij,ij->i", oc, oc) - self.sc[j] ** 2)
                ok = disc > 0.0
                sq = np.sqrt(np.where(ok, disc, 0.0))
                T[:, 2 * j] = np.where(ok, -b - sq, np.inf)
                T[:, 2 * j + 1] = np.where(ok, -b + sq, np.inf)
            else:
                den = d @ self.vec[j]
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = (self.sc[j] - o @ self.vec[j]) / den
                T[:, 2 * j] = np.where(np.isfinite(t), t, np.inf)
        T[~(T > T_MIN)] = np.inf
        order = np.argsort(T, axis=1)
        Ts = np.take_along_axis(T, order, axis=1)
        K = Ts.shape[1]
        hit_k = np.full(n, -1)
        front = np.zeros(n, dtype=bool)
        behind = np.zeros(n)  # a point just behind the hit surface: the midpoint that showed the flip
        act = np.nonzero(np.isfinite(Ts[:, 0]))[0] if K else np.zeros(0, dtype=np.int64)
        state = self.inside(o[act] + d[act] * (0.5 * (T_MIN + Ts[act, 0]))[:, None])
        for k in range(K):
            if not len(act):
                break
            tk = Ts[act, k]
            nxt = Ts[act, k + 1] if k + 1 < K else np.full(len(act), np.inf)
            more = np.isfinite(nxt)
            # coincident roots are one crossing: no midpoint between them
            ask = ~(more & (np.where(more, nxt, 0.0) - tk <= TIE * np.maximum(1.0, tk)))
            mid = np.where(more, 0.5 * (tk + np.where(more, nxt, 0.0)), tk + 1.0)
            after = state.copy()
            after[ask] = self.inside(o[act[ask]] + d[act[ask]] * mid[ask, None])
            flip = after != state
            hit_k[act[flip]] = k
            front[act[flip]] = after[flip]
            behind[act[flip]] = mid[flip]
            keep = ~flip & more
            act, state = act[keep], after[keep]
        hit = hit_k >= 0
        kk = np.where(hit, hit_k, 0)
        rows = np.arange(n)
        t = np.where(hit, Ts[rows, kk], np.inf) if K else np.full(n, np.inf)
        leaf = (order[rows, kk] // 2) if K else np.zeros(n, dtype=np.int64)
        # of coincident roots, the owner is the leaf whose membership decides the flip
        th = np.where(hit, t, 0.0)
        tied = np.nonzero(hit & (kk > 0) & (th - Ts[rows, np.maximum(kk - 1, 0)] <= TIE * np.maximum(1.0, th)))[0] \
            if K else []
        if len(tied):
            leaf_in = self.leaf_membership(o[tied] + d[tied] * behind[tied, None])
            found = np.zeros(len(tied), dtype=bool)
            for back in range(min(K, 4)):
                col = np.maximum(kk[tied] - back, 0)
                cand = order[tied, col] // 2
                ok = ~found & (kk[tied] >= back) & (t[tied] - Ts[tied, col] <= TIE * np.maximum(1.0, t[tied]))
                toggled = [m ^ (ok & (cand == j)) for j, m in enumerate(leaf_in)]
                ok &= self.member(toggled, len(tied)) != front[tied]
                leaf[tied[ok]] = cand[ok]
                found |= ok
        P = o + d * np.where(hit, t, 0.0)[:, None]
        sph = (self.kind[leaf] == 0) if K else np.zeros(n, dtype=bool)
        N = np.where(sph[:, None], (P - self.vec[leaf]) / np.where(sph, self.sc[leaf], 1.0)[:, None], self.vec[leaf]) \
            if K else np.zeros((n, 3))
        N = np.where((np.einsum("ij,ij->i", N, d) > 0.0)[:, None], -N, N)
        return hit, t, N, front, leaf


def _unit_vectors(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _dot(a, b):
    return np.einsum("ij,ij->i", a, b)


def _radiance(scene, rng, o, d, max_depth, mutate):
    """Radiance (n, 3) of the paths that start as (o, d)."""
    n = len(o)
    rad = np.zeros((n, 3))
    ids = np.arange(n)
    thr = np.ones((n, 3))
    dsky = d  # the direction the sky is read from (the unnormalised one under sky_unnormalised)
    segments = max_depth + (1 if mutate == "depth_plus_one" else 0)
    for _ in range(segments):
        if not len(ids):
            break
        hit, t, N, front, leaf = scene.trace(o, d)
        miss = ~hit
        rad[ids[miss]] = thr[miss] * sky(dsky[miss, 1])
        ids, o, d, thr, t, N, front, leaf = ids[hit], o[hit], d[hit], thr[hit], t[hit], N[hit], front[hit], leaf[hit]
        m = len(ids)
        P = o + d * t[:, None]
        kind = scene.mkind[leaf]
        new = np.zeros((m, 3))
        alive = np.ones(m, dtype=bool)
        att = np.ones((m, 3))

        lam = kind == LAMBERTIAN
        if lam.any():
            u = _unit_vectors(rng, int(lam.sum()))
            if mutate == "lambert_uniform":
                s = np.where((_dot(u, N[lam]) < 0.0)[:, None], -u, u)
            else:
                s = N[lam] + u
                tiny = np.linalg.norm(s, axis=1) < 1e-12
                s[tiny] = N[lam][tiny]
            new[lam] = s
            att[lam] = scene.albedo[leaf[lam]]

        met = kind == METAL
        if met.any():
            dm, Nm = d[met], N[met]
            u = _unit_vectors(rng, len(dm))
            if mutate == "fuzz_ball":
                u *= np.cbrt(rng.random(len(dm)))[:, None]
            s = dm - 2.0 * _dot(dm, Nm)[:, None] * Nm + scene.fuzz[leaf[met]][:, None] * u
            if mutate != "metal_no_absorb":
                alive[met] = _dot(s, Nm) > 0.0
            new[met] = s
            att[met] = scene.albedo[leaf[met]]

        die = kind == DIELECTRIC
        if die.any():
            dd, Nd, ior = d[die], N[die], scene.ior[leaf[die]]
            entering = front[die]
            if mutate == "ior_swapped":
                entering = ~entering
            ratio = np.where(entering, 1.0 / ior, ior)
            cos_i = np.minimum(-_dot(dd, Nd), 1.0)
            sin_i = np.sqrt(np.maximum(0.0, 1.0 - cos_i * cos_i))
            tir = ratio * sin_i > 1.0
            if mutate == "no_tir":
                tir[:] = False
            cos_s = cos_i
            if mutate == "schlick_cos_transmitted":
                cos_t = np.sqrt(np.maximum(0.0, 1.0 - (ratio * sin_i) ** 2))
                cos_s = np.where(front[die], cos_i, cos_t)
            refl = schlick(cos_s, ior, 4 if mutate == "schlick_pow4" else 5)
            # a uniform is drawn for every dielectric hit; where refraction is impossible it goes unused,
            # which changes no expectation (3.1 draws it only when refraction is possible)
            reflect = tir | (refl > rng.random(len(dd)))
            perp = ratio[:, None] * (dd + cos_i[:, None] * Nd)
            par = -np.sqrt(np.abs(1.0 - _dot(perp, perp)))
            new[die] = np.where(reflect[:, None], dd - 2.0 * _dot(dd, Nd)[:, None] * Nd, perp + par[:, None] * Nd)

        thr = thr * att
        ids, thr, o, new = ids[alive], thr[alive], P[alive], new[alive]
        d = new / np.linalg.norm(new, axis=1, keepdims=True)
        dsky = new if mutate == "sky_unnormalised" else d
    if mutate == "limit_returns_sky" and len(ids):
        rad[ids] = thr * sky(dsky[:, 1])
    return rad


def render(rec, W, H, spp, max_depth, seed=1, mutate=None, chunk_paths=1 << 16, workers=8):
    """Path-trace the recorded scene.  Returns (mean, variance, n): per pixel and channel the
    mean radiance (H, W, 3), the per-sample variance (H, W, 3) and the sample count."""
    assert mutate is None or mutate in MUTANTS, mutate
    scene = rec if isinstance(rec, Scene) else Scene(rec)
    cam = Camera(scene.cam, W, H)
    mean = np.zeros((H * W, 3))
    var = np.zeros((H * W, 3))
    step = max(1, chunk_paths // spp)

    def chunk(c, p0):
        rng = np.random.default_rng([seed, c])
        pix = np.arange(p0, min(p0 + step, W * H))
        pid = np.repeat(pix, spp)
        n = len(pid)
        px, py = (pid % W).astype(np.float64), (pid // W).astype(np.float64)
        if mutate == "no_jitter":
            jx = jy = np.full(n, 0.5)
        else:
            jx, jy = rng.random(n), rng.random(n)
        lens = None
        if cam.lens_radius > 0.0:
            u, phi = rng.random(n), 2.0 * math.pi * rng.random(n)
            r = u if mutate == "lens_r_linear" else np.sqrt(u)
            lens = np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1)
        o, d = cam.rays(px, py, jx, jy, lens, row_flip=(mutate == "row_flip"))
        rad = _radiance(scene, rng, o, d, max_depth, mutate).reshape(len(pix), spp, 3)
        mean[pix] = rad.mean(axis=1)
        var[pix] = rad.var(axis=1, ddof=1) if spp > 1 else 0.0

    # each chunk has its own stream, so the result does not depend on the number of threads
    with ThreadPoolExecutor(max_workers=max(1, workers)) as pool:
        list(pool.map(lambda a: chunk(*a), enumerate(range(0, W * H, step))))
    return mean.reshape(H, W, 3), var.reshape(H, W, 3), spp
