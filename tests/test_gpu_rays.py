"""GPU: batched ray queries and picking (wo_renderer_trace_rays*, wo_renderer_pick) against
the CPU oracle's trace query (pyoracle.trace), bit for bit: hit / miss, t, the hit leaf's
record, the node it was compiled from, the solid's outward normal and the material."""
import numpy as np
import pytest

import pyoracle
from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl

pytestmark = pytest.mark.gpu

HIT_DT = np.dtype(wl.RAY_HIT_FIELDS)
N_RAYS = 4099  # no multiple of 64 or 256
# where group (b)'s origins are drawn: each scene's geometry and a margin
BOXES = {
    "csg32": ((-6.5, -1.0, -6.5), (6.5, 3.0, 6.5)),
    "csg32_union": ((-6.5, -1.0, -6.5), (6.5, 3.0, 6.5)),
    "csg32_nested": ((-3.0, -1.2, -3.0), (3.0, 4.4, 3.0)),
    "rtiow_cover": ((-11.0, -0.5, -11.0), (11.0, 2.5, 11.0)),
}
SEEDS = {"csg32": 101, "csg32_union": 102, "csg32_nested": 103, "rtiow_cover": 104}
LANE_FORMS = {"csg32_union": 2, "rtiow_cover": 3}  # wo_dev_impl.h PathKind of the lane walk
CASES = [(s, "interpreter") for s in BOXES] + [(s, "lanes") for s in LANE_FORMS]


def _renderer(scene):
    r = wl.Renderer(scene, max_nodes=4096)
    scenes.build(scene, r)
    r.set_tracer("interpreter")  # the frames' kernel: ray queries never use the specialised one
    return r


def _unit(v):
    """float32 rows normalised in float32."""
    v = np.asarray(v, dtype=np.float32)
    n = np.sqrt((v * v).sum(axis=1, dtype=np.float32), dtype=np.float32)
    return (v / n[:, None]).astype(np.float32)


def _rows(o, d, t_max=np.inf):
    rays = np.zeros((len(o), 8), dtype=np.float32)
    rays[:, 0:3] = o
    rays[:, 3] = t_max
    rays[:, 4:7] = d
    return rays


class Scene:
    """The compiled scene as the oracle needs it, and expected Wo_RayHit rows from it."""

    def __init__(self, r):
        self.prog, self.nrec, self.nprims = r.program()
        self.nodes = r.program_nodes()
        self.n_mats = r.materials()[1]
        self.ordpc = {self.prog[pc].u1: pc for pc in range(self.nrec) if self.prog[pc].op == wl.WO_OP_PRIM}
        self.op = np.array([self.prog[i].op for i in range(self.nrec)], dtype=np.uint32)
        self.u0 = np.array([self.prog[i].u0 for i in range(self.nrec)], dtype=np.uint32)
        self.f = np.array([[self.prog[i].f[k] for k in range(5)] for i in range(self.nrec)], dtype=np.float32)

    def expect(self, rays):
        """Expected hits of an (n, 8) float32 batch: pyoracle.trace per ray, then the normal as
        oracle.c shade_pixel forms it, restated in float32 (one rounding per operation)."""
        rays = np.asarray(rays, dtype=np.float32)
        n = len(rays)
        exp = np.zeros(n, dtype=HIT_DT)
        exp["t"] = np.inf
        exp["leaf"] = exp["node"] = exp["material"] = 0xFFFFFFFF
        typ = np.zeros(n, dtype=np.uint32)
        after = np.zeros(n, dtype=np.uint32)
        for i in range(n):
            o, d, t_max = rays[i, 0:3], rays[i, 4:7], rays[i, 3]
            valid = np.isfinite(o).all() and np.isfinite(d).all() and bool((d != 0).any()) and not np.isnan(t_max)
            if not valid:
                exp["flags"][i] = wl.RAY_INVALID
                continue
            res = pyoracle.trace(self.prog, self.nrec, o, d)
            if res is None or not np.float32(res[0]) <= t_max:
                continue
            t, prim, ty, member, ra = res
            leaf = self.ordpc[prim] + 1 + member
            exp["t"][i] = t
            exp["flags"][i] = wl.RAY_HIT | (wl.RAY_EXIT if ty else 0) | (wl.RAY_ENTERS if ra else 0)
            exp["leaf"][i] = leaf
            typ[i], after[i] = ty, ra
        hit = (exp["flags"] & wl.RAY_HIT) != 0
        leaf = exp["leaf"][hit]
        assert np.isin(self.op[leaf], (wl.WO_LEAF_SPHERE, wl.WO_LEAF_HALFSPACE)).all()
        exp["node"][hit] = self.nodes[leaf]
        exp["material"][hit] = np.where(self.u0[leaf] < self.n_mats, self.u0[leaf], 0)
        o, d, t = rays[hit, 0:3], rays[hit, 4:7], exp["t"][hit]
        P = o + t[:, None] * d  # float32: a product, then a sum
        f = self.f[leaf]
        nl = np.where((self.op[leaf] == wl.WO_LEAF_SPHERE)[:, None], (P - f[:, 0:3]) * f[:, 4:5], f[:, 0:3])
        N = np.where((typ[hit] == 0)[:, None], nl, -nl)
        exp["normal"][hit] = np.where((after[hit] != 0)[:, None], N, -N).astype(np.float32)
        return exp


def make_batch(r, scene, n=N_RAYS, nb=1500, step=3, box=None, seed=None):
    """The seeded batch of a scene (no device needed): (a) pixel rays of a coarse grid (every
    `step`-th pixel), (b) `nb` origins uniform in the scene's box with uniform directions, (c)
    origins on the surface (the oracle's hit points of (a)) with uniform directions, (d)
    axis-parallel directions.  `box` and `seed` stand in for a scene BOXES / SEEDS do not list."""
    sc = Scene(r)
    rng = np.random.default_rng(SEEDS[scene] if seed is None else seed)
    lo, hi = (np.array(v, dtype=np.float64) for v in (box or BOXES[scene]))
    p = wl.render_params(96, 54, mode=wl.MODE_NORMALS)
    a = np.stack([r.pixel_ray(p, x, y) for y in range(1, 54, step) for x in range(1, 96, step)])
    b = _rows(rng.uniform(lo, hi, size=(nb, 3)), _unit(rng.normal(size=(nb, 3))))
    ea = sc.expect(a)
    oc = rng.uniform(lo, hi, size=(len(a), 3)).astype(np.float32)
    on = (ea["flags"] & wl.RAY_HIT) != 0
    oc[on] = a[on, 0:3] + ea["t"][on][:, None] * a[on, 4:7]
    c = _rows(oc, _unit(rng.normal(size=(len(a), 3))))
    nd = n - len(a) - nb - len(c)
    axes = np.zeros((nd, 3), dtype=np.float32)
    axes[np.arange(nd), rng.integers(0, 3, size=nd)] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=nd)
    d = _rows(rng.uniform(lo, hi, size=(nd, 3)), axes)
    rays = np.concatenate([a, b, c, d]).astype(np.float32)
    assert rays.shape == (n, 8)
    exp = np.concatenate([ea, sc.expect(rays[len(a):])])
    return sc, rays, exp


def batch_is_telling(exp):
    """Judged on the oracle's results alone: enough hits, misses and exits from the solid."""
    n = len(exp)
    hit = (exp["flags"] & wl.RAY_HIT) != 0
    leaving = hit & ((exp["flags"] & wl.RAY_ENTERS) == 0)
    return {"hit": hit.sum() / n, "miss": (~hit).sum() / n, "root_after_0": leaving.sum() / n,
            "exit_events": (hit & ((exp["flags"] & wl.RAY_EXIT) != 0)).sum() / n}


_BATCHES = {}


def _batch(r, scene):
    if scene not in _BATCHES:  # the oracle's pass is made once per scene and shared
        sc, rays, exp = make_batch(r, scene)
        exp.setflags(write=False)
        rays.setflags(write=False)
        _BATCHES[scene] = (sc, rays, exp)
    return _BATCHES[scene]


def _same(got, exp, what):
    assert got.dtype == HIT_DT and got.shape == exp.shape, what
    bad = {}
    for name in HIT_DT.names:
        g = np.ascontiguousarray(got[name]).view(np.uint32)
        e = np.ascontiguousarray(exp[name]).view(np.uint32)
        nbad = int((g != e).reshape(len(got), -1).any(axis=1).sum())
        if nbad:
            first = int(np.flatnonzero((g != e).reshape(len(got), -1).any(axis=1))[0])
            bad[name] = (nbad, first, got[first], exp[first])
    assert not bad, f"{what}: not bit-exact: {bad}"


def _device_form(r, rays):
    import torch
    d_rays = torch.from_numpy(np.array(rays, dtype=np.float32)).cuda()  # (a writable copy of the shared batch)
    d_hits = torch.zeros((len(rays), 32), dtype=torch.uint8, device="cuda")
    r.trace_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), len(rays), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_hits.cpu().numpy().reshape(-1).view(HIT_DT)


def _check_path(r, scene, path):
    assert r.ray_path() == path
    if path == "lanes":
        assert r.lanes_info()["kind"] == LANE_FORMS[scene]


@pytest.mark.parametrize("scene,path", CASES)
def test_rays_bitexact_vs_oracle(scene, path, monkeypatch):
    r = _renderer(scene)
    sc, rays, exp = _batch(r, scene)
    telling = batch_is_telling(exp)
    print(scene, telling)
    assert telling["hit"] >= 0.25 and telling["miss"] >= 0.05 and telling["root_after_0"] >= 0.05, telling
    assert r.ray_path() == "none"
    r.set_ray_tracer(path)
    host = r.trace_rays(rays)
    _check_path(r, scene, path)
    _same(host, exp, f"{scene} {path} host form")
    dev = _device_form(r, rays)
    _check_path(r, scene, path)
    assert dev.tobytes() == host.tobytes(), f"{scene} {path}: device form differs from the host form"
    # two workgroups: nine trips of the grid-stride loop, the last one partial
    monkeypatch.setenv("WOLOLO_RAY_BLOCKS", "2")
    _same(r.trace_rays(rays), exp, f"{scene} {path} two workgroups")
    r.close()


@pytest.mark.parametrize("scene,path", [("csg32", "interpreter"), ("csg32_union", "interpreter"),
                                        ("csg32_union", "lanes")])
def test_ray_results_are_independent_of_the_batch(scene, path):
    """Prefixes (tail lanes, n = 0) and a permutation (other wave-mates) give the same rows."""
    r = _renderer(scene)
    _, rays, exp = _batch(r, scene)
    r.set_ray_tracer(path)
    full = r.trace_rays(rays)
    _same(full, exp, f"{scene} {path}")
    for n in (0, 1, 63, 64, 65, 257):
        got = r.trace_rays(rays[:n])
        assert len(got) == n and got.tobytes() == full[:n].tobytes(), (scene, path, n)
    perm = np.random.default_rng(7).permutation(len(rays))
    got = r.trace_rays(rays[perm])
    assert got.tobytes() == full[perm].tobytes(), (scene, path, "permutation")
    _check_path(r, scene, path)
    r.close()


@pytest.mark.parametrize("scene,path", [("csg32", "interpreter"), ("csg32_union", "lanes")])
def test_t_max_bounds_the_hit(scene, path):
    r = _renderer(scene)
    sc, rays, exp = _batch(r, scene)
    r.set_ray_tracer(path)
    sel = np.flatnonzero((exp["flags"] & wl.RAY_HIT) != 0)[:320]
    assert len(sel) >= 200
    at = rays[sel].copy()
    at[:, 3] = exp["t"][sel]  # t_max = t: still the hit
    _same(r.trace_rays(at), exp[sel], f"{scene} {path} t_max = t")
    below = rays[sel].copy()
    below[:, 3] = np.nextafter(exp["t"][sel], np.float32(0))
    miss = sc.expect(below)
    assert (miss["flags"] == 0).all() and np.isinf(miss["t"]).all() and (miss["leaf"] == 0xFFFFFFFF).all()
    _same(r.trace_rays(below), miss, f"{scene} {path} t_max below t")
    r.close()


def _spoil(rays, rows):
    """Make `rows` (12 of them) invalid, each in another way."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    ways = [(0, nan), (1, inf), (2, -inf), (4, nan), (5, inf), (6, -inf), (3, nan), (1, nan), (6, inf)]
    for row, (col, v) in zip(rows, ways):
        rays[row, col] = v
    rays[rows[9], 4:7] = 0.0                    # dir == 0
    rays[rows[10], 4:7] = (-0.0, 0.0, -0.0)     # and with signed zeros
    rays[rows[11], :] = nan
    return rays


@pytest.mark.parametrize("scene,path", [("csg32", "interpreter"), ("csg32_union", "lanes")])
def test_invalid_rays_are_reported_not_traced(scene, path):
    r = _renderer(scene)
    sc, rays, exp = _batch(r, scene)
    r.set_ray_tracer(path)
    rows = [0, 3, 9, 17, 18, 31, 40, 41, 55, 62, 63, 66]  # lane 0 and lane 63 of the first wave among them
    some = _spoil(rays[600:670].copy(), rows)
    want = sc.expect(some)
    assert (want["flags"][rows] == wl.RAY_INVALID).all() and (want["flags"] != wl.RAY_INVALID).sum() == 58
    assert np.isinf(want["t"][rows]).all() and (want["node"][rows] == 0xFFFFFFFF).all()
    keep = np.setdiff1d(np.arange(70), rows)
    assert want[keep].tobytes() == exp[600:670][keep].tobytes()
    _same(r.trace_rays(some), want, f"{scene} {path} 12 invalid of 70")
    # a whole wave of invalid rays between two valid ones
    more = rays[600:800].copy()
    more[64:128, 4:7] = 0.0
    want = sc.expect(more)
    assert (want["flags"][64:128] == wl.RAY_INVALID).all()
    _same(r.trace_rays(more), want, f"{scene} {path} an invalid wave")
    r.close()


def test_pick_and_normals_frame_agree():
    r = _renderer("csg32")
    sc = Scene(r)
    w, h = 96, 54
    p = wl.render_params(w, h, spp=1, max_depth=1, mode=wl.MODE_NORMALS)
    rng = np.random.default_rng(2024)
    xs, ys = rng.integers(0, w, size=200), rng.integers(0, h, size=200)
    rays = np.stack([r.pixel_ray(p, x, y) for x, y in zip(xs, ys)])
    exp = sc.expect(rays)
    got = np.array([r.pick(p, x, y) for x, y in zip(xs, ys)], dtype=HIT_DT)
    _same(got, exp, "pick")
    mats, nm = r.materials()
    pix, _ = pyoracle.pathtrace_pixels(sc.prog, sc.nrec, mats, nm, r.frame_desc(p), xs, ys)
    hit = (got["flags"] & wl.RAY_HIT) != 0
    assert 20 <= hit.sum() <= 190
    shaded = np.float32(0.5) * (got["normal"][hit] + np.float32(1.0))
    assert shaded.dtype == np.float32 and shaded.tobytes() == np.ascontiguousarray(pix[hit, :3]).tobytes()
    t = np.float32(0.5) * (rays[~hit, 5] + np.float32(1.0))  # the oracle's sky gradient
    s = np.float32(1.0) - t
    sky = np.stack([s + t * np.float32(0.5), s + t * np.float32(0.7), s + t * np.float32(1.0)], axis=1)
    assert sky.dtype == np.float32 and sky.tobytes() == np.ascontiguousarray(pix[~hit, :3]).tobytes()
    wl.clear_error()
    with pytest.raises(wl.WololoError, match="outside"):
        r.pick(p, w, 0)
    r.close()


def test_rays_follow_a_scene_edit():
    r = wl.Renderer("edit", max_nodes=4096)
    scenes.build("csg32", r)
    r.set_tracer("interpreter")
    p = wl.render_params(96, 54, mode=wl.MODE_NORMALS)
    rays = np.stack([r.pixel_ray(p, x, y) for y in range(2, 54, 4) for x in range(2, 96, 4)])
    before = Scene(r)
    exp0 = before.expect(rays)
    _same(r.trace_rays(rays), exp0, "before the edit")
    # a sphere in front of the camera (which looks from (0, 4.5, 10) at (0, 0.6, 0)), unioned in
    ball = r.sphere(0.8)
    r.union(wl.arg(ball, (0.0, 3.4, 7.2)), wl.arg(ball, (0.3, 3.4, 7.2)))
    after = Scene(r)
    assert after.nrec > before.nrec
    exp1 = after.expect(rays)
    got = r.trace_rays(rays)
    _same(got, exp1, "after the edit")
    on_ball = got["node"] == ball
    assert on_ball.sum() >= 20 and (exp0["node"] != ball).all()
    assert (after.op[got["leaf"][on_ball]] == wl.WO_LEAF_SPHERE).all()
    assert (after.nodes[got["leaf"][on_ball]] == ball).all()
    r.close()
