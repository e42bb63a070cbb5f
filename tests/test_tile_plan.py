"""The path tracer's tile planner (trace_kernels.hip plan_tiles, through wo_plan_tiles) on
the CPU: which pixels each workgroup renders.  The kernel's decode of a workgroup index
(wo_device_common.h pathtrace_block) is restated here: workgroups below n_big are big
tiles, tiles_x_big to a row, from local row 0; the rest are small tiles, tiles_x_small to
a row, from local row rows_big; a shape is log2 width | log2 height << 4.  No GPU."""
import functools
import hashlib
import itertools
import struct

import numpy as np
import pytest

from csgrenderer_amd import wololo as wl

K_TILE_MAX_PIX = 64  # wo_device_common.h kTileMaxPix: a tile's pixels are lanes of one wave

WIDTHS = (1, 3, 7, 8, 9, 16, 17, 63, 64, 65, 127, 200, 1920)
ROWS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 31, 33, 64, 100, 135, 270, 1080)
RESIDENT = (1, 2, 7, 64, 256, 1024, 2048, 8192)
BAND_ROWS = (1, 2, 4, 8, 16, 0xFFFFFFFF)
WANT = (1, 3, 8, 64)
# SHA-256 of the seven outputs (little-endian uint32) over the grid in the order above,
# from the planner and launch_impl's workgroup arithmetic as they stood before the
# workgroup count moved into the planner (their text compiled into a host program)
PLANS_SHA256 = "c7ba462eeef8af8fddb2e5e7a424c9f7f0dcf7d7d7ec1814147ab38305503991"


@pytest.fixture()
def plain_planner(monkeypatch):
    for name in ("WOLOLO_TILE", "WOLOLO_TILE_WANT", "WOLOLO_TILE_SPAN"):
        monkeypatch.delenv(name, raising=False)


@functools.lru_cache(maxsize=None)
def _columns(width, big_w, tiles_x_big, small_w, tiles_x_small):
    """Per pixel column: in a big tile, in a small tile (a tile column txi covers
    x in [txi << w, (txi + 1) << w))."""
    x = np.arange(width)
    cb, cs = (x >> big_w) < tiles_x_big, (x >> small_w) < tiles_x_small
    return bool(cb.all()), bool(cs.all()), bool((cb ^ cs).all())


@functools.lru_cache(maxsize=None)
def _rows(rows, big_h, tile_rows_big, rows_big, small_h, tile_rows_small):
    """Per local row: in a big tile row, in a small tile row (from rows_big on)."""
    y = np.arange(rows)
    rb = (y >> big_h) < tile_rows_big
    rs = (y >= rows_big) & (((y - rows_big) >> small_h) < tile_rows_small)
    return bool((rb & ~rs).any()), bool((rs & ~rb).any()), bool((rb & rs).any()), bool((~rb & ~rs).any())


def test_every_pixel_in_exactly_one_tile(plain_planner):
    """Every pixel with x < width and local row < rows lies in exactly one tile, and no
    tile has more than kTileMaxPix pixels.  Each region's grid is a product of a
    column and a row partition, so a count per column and per row decides it.  The
    seven outputs over the whole grid are pinned by their digest."""
    digest = hashlib.sha256()
    for width, rows, resident, band, want in itertools.product(WIDTHS, ROWS, RESIDENT, BAND_ROWS, WANT):
        case = (width, rows, resident, band, want)
        plan = wl.plan_tiles(*case)
        assert plan is not None, case
        digest.update(struct.pack("<7I", *plan))
        big, small, n_big, txb, txs, rows_big, n_wg = plan
        for shape in (big, small):
            assert 1 << ((shape & 15) + (shape >> 4)) <= K_TILE_MAX_PIX, (case, plan)
        assert txb > 0 and txs > 0 and n_big % txb == 0 and n_wg >= n_big and (n_wg - n_big) % txs == 0, (case, plan)
        all_big, all_small, one_of = _columns(width, big & 15, txb, small & 15, txs)
        only_big, only_small, both, neither = _rows(rows, big >> 4, n_big // txb, rows_big, small >> 4,
                                                    (n_wg - n_big) // txs)
        assert not neither, (case, plan, "a row in no tile")
        assert all_big or not only_big, (case, plan, "a column of a big-tile row in no tile")
        assert all_small or not only_small, (case, plan, "a column of a small-tile row in no tile")
        assert one_of or not both, (case, plan, "a pixel in a big and a small tile, or in neither")
    assert digest.hexdigest() == PLANS_SHA256
