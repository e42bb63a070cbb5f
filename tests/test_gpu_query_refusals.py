"""GPU: what the device-pointer forms of the queries refuse, and in which words.  Every call here is
refused before any launch, so nothing runs on the device; the buffers are real device memory, passed
4 bytes off.  Each text is the one of the layer that answers: query_launch.hip's for the ray, span,
point and mass buffers, renderer.c's features_args for the planes (it checks the buffer and the
stride before wo_dev_features, whose own "the planes' buffer must be device memory, 16-byte
aligned" no caller of the public API can reach), mass.c's for the grid's axis."""
import pytest

import test_gpu_rays as tgr
from csgrenderer_amd import scenes
from csgrenderer_amd import wololo as wl

pytestmark = pytest.mark.gpu

BOX = tgr.BOXES["csg32_union"]


@pytest.fixture(scope="module")
def scene():
    """csg32_union (a node table and a lane form) and 4 KiB of device memory."""
    import torch
    r = wl.Renderer("refusals", max_nodes=4096)
    info = scenes.build("csg32_union", r)
    buf = torch.zeros(1024, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    yield r, info, buf.data_ptr()
    r.close()


def _refused(text, call, *args):
    with pytest.raises(wl.WololoError) as e:
        call(*args)
    assert text in str(e.value), str(e.value)


def test_misaligned_ray_buffers(scene):
    r, _, d = scene
    _refused("ray and hit buffers must be 16-byte aligned", r.trace_rays_device, d + 4, d + 256, 1)
    _refused("ray and hit buffers must be 16-byte aligned", r.trace_rays_device, d, d + 256 + 4, 1)


def test_misaligned_span_buffers(scene):
    r, _, d = scene
    for off in ((4, 0, 0), (0, 4, 0), (0, 0, 4)):
        _refused("ray, span and crossing buffers must be 16-byte aligned", r.trace_spans_device, d + off[0],
                 d + 256 + off[1], d + 512 + off[2], 1, 1)


def test_misaligned_point_buffer(scene):
    r, _, d = scene
    _refused("the point buffer must be 16-byte aligned", r.classify_points_device, d + 4, d + 256, 1)


def test_misaligned_sums_buffer(scene):
    r, _, d = scene
    g = wl.mass_grid(*BOX, 0, 1, 1)
    _refused("the sums' buffer must be device memory, 8-byte aligned", r.mass_sums_device, g, d + 4)


def test_bad_mass_axis(scene):
    """mass.c answers before the device layer's "bad mass grid"."""
    r, _, d = scene
    g = wl.mass_grid(*BOX, 0, 1, 1)
    g.axis = 3
    _refused("mass grid: axis 3 (0, 1 or 2)", r.mass_sums_device, g, d)


def test_misaligned_planes_buffer(scene):
    r, info, d = scene
    p = info.params(width=1, height=1, spp=1)
    _refused("the buffer is NULL or not 16-byte aligned", r.render_features_device, p, d + 4, 1, 1, 0, 1)


def test_zero_plane_stride(scene):
    r, info, d = scene
    p = info.params(width=1, height=1, spp=1)
    _refused("plane_stride 0 is short of the rank's 1 rows x 1 pixels", r.render_features_device, p, d, 0, 1, 0, 1)

