"""Ray queries and picking, the host side (CPU only): the record -> node table of the scene
compiler, the Wo_Ray / Wo_RayHit layout, the pixel ray, and the loud failure without a device."""
import ctypes
import math

import numpy as np
import pytest

from csgrenderer_amd import wololo as wl


def _quat(axis, deg):
    h = math.radians(deg) / 2.0
    s = math.sin(h)
    return wl.Quaternion(math.cos(h), wl.vec3(axis[0] * s, axis[1] * s, axis[2] * s))


def _rotate(q, v):
    """v rotated by the unit quaternion q (float64)."""
    w = q.real
    u = np.array([q.imaginary.x, q.imaginary.y, q.imaginary.z])
    v = np.asarray(v, dtype=np.float64)
    return v + 2.0 * w * np.cross(u, v) + 2.0 * np.cross(u, np.cross(u, v))


def test_program_nodes_name_each_leaf(hostonly):
    """One sphere node instanced twice, a rotated box of six half-space nodes, and a
    difference: every leaf record names the node it was compiled from."""
    r = wl.Renderer("nodes", max_nodes=64)
    ball = r.sphere(1.0)
    pair = r.union(wl.arg(ball, (-3.0, 0.0, 0.0)), wl.arg(ball, (3.0, 0.5, 0.0)))  # the same node twice
    normals = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    planes = [r.halfspace(n) for n in normals]
    box = None
    for n, h in zip(normals, planes):  # each plane pushed 0.8 along its normal
        a = wl.arg(h, tuple(0.8 * c for c in n))
        box = a if box is None else wl.arg(r.intersection(box, a))
    turn = _quat((0.0, 0.0, 1.0), 30.0)
    dent = r.sphere(0.6)
    dented = r.difference(wl.NodeArgument(turn, wl.vec3(0.0, 4.0, 0.0), box.node), wl.arg(dent, (0.0, 4.8, 0.0)))
    assert r.isroot(pair) and r.isroot(dented)

    n_recs = r.compile()
    prog, nr, _ = r.program()
    nodes = r.program_nodes()
    assert nr == n_recs and len(nodes) == n_recs
    spheres, halves = [], []
    for i in range(n_recs):
        op = prog[i].op
        if op == wl.WO_LEAF_SPHERE:
            spheres.append((i, int(nodes[i])))
        elif op == wl.WO_LEAF_HALFSPACE:
            halves.append((i, int(nodes[i])))
        else:
            assert nodes[i] == wl.WO_NODE_INVALID, (i, op)
    # three sphere leaves: the ball twice (both instances name the same handle), the dent once
    assert sorted(n for _, n in spheres) == [ball, ball, dent]
    for i, n in spheres:
        want_r2 = 1.0 if n == ball else 0.36
        assert prog[i].f[3] == pytest.approx(want_r2, rel=1e-6)
    centres = sorted(tuple(round(prog[i].f[k], 5) for k in range(3)) for i, n in spheres if n == ball)
    assert centres == [(-3.0, 0.0, 0.0), (3.0, 0.5, 0.0)]
    # six half-space leaves, each naming the node whose normal, rotated, is the record's
    assert sorted(n for _, n in halves) == sorted(planes)
    for i, n in halves:
        want = _rotate(turn, normals[planes.index(n)])
        got = np.array([prog[i].f[k] for k in range(3)], dtype=np.float64)
        assert np.allclose(got, want, atol=1e-6), (i, n, got, want)
    r.close()


@pytest.mark.parametrize("cname,mirror", [("Wo_Ray", wl.Ray), ("Wo_RayHit", wl.RayHit)])
def test_ray_abi_layout(cname, mirror):
    assert ctypes.sizeof(mirror) == 32
    assert wl.abi_layout(cname) == 32
    for fname, _ in mirror._fields_:
        assert wl.abi_layout(cname, fname) == getattr(mirror, fname).offset, (cname, fname)
    # the numpy view trace_rays returns has the same layout
    if mirror is wl.RayHit:
        dt = np.dtype(wl.RAY_HIT_FIELDS)
        assert dt.itemsize == 32
        for fname, _ in mirror._fields_:
            assert dt.fields[fname][1] == getattr(mirror, fname).offset, fname


def test_trace_rays_without_device_fails_loudly(hostonly):
    r = wl.Renderer("nodev", max_nodes=4)
    r.sphere(1.0)
    p = wl.render_params(8, 8, mode=wl.MODE_NORMALS)
    rays = np.zeros((3, 8), dtype=np.float32)
    rays[:, 6] = -1.0
    for call in (lambda: r.trace_rays(rays), lambda: r.trace_rays_device(0x1000, 0x2000, 3), lambda: r.pick(p, 4, 4)):
        wl.clear_error()
        with pytest.raises(wl.WololoError, match="device"):
            call()
    assert r.lib.wo_renderer_trace_rays(r.ptr, rays.ctypes.data, rays.ctypes.data, 3) == -1
    assert r.ray_path() == "none"
    ray = r.pixel_ray(p, 4, 4)  # host arithmetic: no device needed
    assert ray.shape == (8,) and np.isfinite(ray[:3]).all() and np.isfinite(ray[4:7]).all()
    r.close()


def test_pixel_ray_is_unit_and_centred(hostonly):
    r = wl.Renderer("ray", max_nodes=4)
    look_from, look_at = np.array([13.0, 2.0, 3.0]), np.array([0.5, 0.25, -1.0])
    r.set_camera(tuple(look_from), tuple(look_at), (0, 1, 0), 20.0, 0.1, 10.0)  # the aperture is ignored
    w, h = 97, 55
    p = wl.render_params(w, h, mode=wl.MODE_NORMALS)
    ulp = float(np.spacing(np.float32(1.0)))
    for x, y in [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2), (17, 41)]:
        ray = r.pixel_ray(p, x, y)
        assert np.isfinite(ray[:3]).all() and np.isfinite(ray[4:7]).all()
        assert ray[3] == np.inf and ray.view(np.uint32)[7] == 0
        assert np.array_equal(ray[:3], look_from.astype(np.float32))
        norm = math.sqrt(sum(float(c) ** 2 for c in ray[4:7]))
        assert abs(norm - 1.0) <= 2 * ulp, (x, y, norm)
    axis = (look_at - look_from) / np.linalg.norm(look_at - look_from)
    centre = r.pixel_ray(p, w // 2, h // 2)[4:7].astype(np.float64)
    assert np.abs(centre - axis).max() < 1e-6
    # a corner ray leans away from the axis by about half the field of view
    corner = r.pixel_ray(p, w // 2, 0)[4:7].astype(np.float64)
    assert math.degrees(math.acos(float(corner @ axis))) == pytest.approx(10.0 * (h - 1) / h, abs=0.2)
    for x, y in [(w, 0), (0, h), (2 ** 32 - 1, 0)]:
        wl.clear_error()
        with pytest.raises(wl.WololoError, match="outside"):
            r.pixel_ray(p, x, y)
    r.close()
