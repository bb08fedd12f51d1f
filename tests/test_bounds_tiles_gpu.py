"""ocean_build_bounds_tiles on the MI355X: the min/max pyramids of a tile range, built in at most two launches, carry exactly the bits of
tests/bounds.py::pyramid of the displacement maps the same frame read out, tile by tile, on every level from first_level up.  Tile sizes
16 (one launch, a block smaller than 64), 64 (exactly one full block), 128 (four blocks, then a second launch on a 2 x 2 source) and 4096
(a full 64 x 64 source in the second launch)."""
import ctypes as C

import numpy as np
import pytest

import bounds as B

pytestmark = pytest.mark.gpu
TILES = 4
RANGES = ((0, 4), (1, 2), (3, 1))
E_INVALID, E_NOT_READY = -1, -4


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def batch(n, tiles=TILES, depth=1):
    import watersurfacerendering_amd as W
    b = W.OceanBatch(n, tiles, 0)
    if depth > 1:
        b.set_pipeline_depth(depth)
    for i in range(tiles):
        b.set_params(tile=i, tile_length=1000.0 / (i + 1), wind_speed=20.0 + 3.0 * i)
    b.prepare(0x5EED0000 + n)
    return b


def read_code(b, tile):
    n = int(b._L.ocean_mip_texels(b.tile_size))
    lo = np.empty((n, 4), np.float32)
    return b._L.ocean_read_bounds_tile(b._h, tile, lo.ctypes.data_as(C.c_void_p), None)


def check_range(b, first, count, first_level, disp):
    b.build_bounds_tiles(first, count, first_level)
    top = b.tile_size.bit_length() - 1
    for tile in range(first, first + count):
        got = b.read_bounds_tile(tile)
        want = B.pyramid(disp[tile])
        assert len(got) == len(want) == top
        for l in range(max(1, first_level), top + 1):
            assert same_bits(got[l - 1][0], want[l - 1][0]), (first, count, first_level, tile, l, "lo")
            assert same_bits(got[l - 1][1], want[l - 1][1]), (first, count, first_level, tile, l, "hi")


@pytest.mark.parametrize("n", [16, 64, 128])
def test_every_stored_level_of_every_tile_is_the_pyramid(n):
    b = batch(n)
    b.compute_waves(1.25)
    disp, _ = b.read_maps()
    top = n.bit_length() - 1
    for first, count in RANGES:
        for first_level in (1, 3, top):
            check_range(b, first, count, first_level, disp)
            assert b.device_bounds_tiles()[2:] == (first, count, top, first_level)
            assert all(b.device_bounds_tiles()[:2])
    check_range(b, 0, TILES, 0, disp)                   # 0 means 1
    assert b.device_bounds_tiles()[5] == 1
    if n == 128:                                        # first_level 7 > 6: the second launch still finds its level 6
        check_range(b, 1, 2, 7, disp)
    b.close()


def test_a_smaller_range_after_a_larger_one():
    b = batch(64)
    b.compute_waves(0.5)
    disp, _ = b.read_maps()
    check_range(b, 0, 4, 1, disp)
    check_range(b, 2, 1, 2, disp)
    for tile in (0, 1, 3):
        assert read_code(b, tile) == E_NOT_READY, tile
    assert read_code(b, 2) == 0
    # both output pointers are optional
    assert b._L.ocean_read_bounds_tile(b._h, 2, None, None) == 0
    b.close()


@pytest.mark.parametrize("depth", [2, 3])
def test_the_set_belongs_to_the_most_recent_frame_at_depth(depth):
    b = batch(128, depth=depth)
    for k in range(depth + 1):      # frames in flight on every chain; the last one is the one the set is built from
        b.compute_waves_async(0.5 + 0.75 * k)
    b.build_bounds_tiles(0, TILES)
    disp, _ = b.read_maps()
    for tile in range(TILES):
        for l, ((glo, ghi), (wlo, whi)) in enumerate(zip(b.read_bounds_tile(tile), B.pyramid(disp[tile])), start=1):
            assert same_bits(glo, wlo) and same_bits(ghi, whi), (depth, tile, l)
    # and again behind one more frame, on the next chain
    b.compute_waves_async(9.0)
    b.build_bounds_tiles(1, 2, 2)
    disp2, _ = b.read_maps()
    assert not np.array_equal(disp2[1], disp[1])
    for tile in (1, 2):
        for l, ((glo, ghi), (wlo, whi)) in enumerate(zip(b.read_bounds_tile(tile), B.pyramid(disp2[tile])), start=1):
            assert l < 2 or (same_bits(glo, wlo) and same_bits(ghi, whi)), (depth, tile, l)
    b.close()


def _patch_code(b, first=0, cascades=1):
    rects = np.zeros((2, 4), np.float32)
    lo, hi = np.empty((2, 4), np.float32), np.empty((2, 4), np.float32)
    s = b._surface(first, [1.0] * cascades, 16, 1.0, 0.0, 0)
    q = b._patch_query(None, 0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return b._L.ocean_patch_bounds(b._h, C.byref(s), C.byref(q), p(rects), 2, p(lo), p(hi))


def test_staleness_and_error_cases():
    import watersurfacerendering_amd as W
    L = W._abi.lib()
    assert L.ocean_build_bounds_tiles(None, 0, 1, 1) == E_INVALID
    assert L.ocean_read_bounds_tile(None, 0, None, None) == E_INVALID
    assert L.ocean_device_bounds_tiles(None, None, None, None, None, None, None) == E_INVALID
    b = W.OceanBatch(16, TILES, 0)
    assert L.ocean_build_bounds_tiles(b._h, 0, 1, 1) == E_NOT_READY         # no Prepare
    b.prepare(0x5EED0010)
    assert L.ocean_build_bounds_tiles(b._h, 0, 1, 1) == E_NOT_READY         # no frame
    assert read_code(b, 0) == E_NOT_READY
    assert b.device_bounds_tiles() == (None, None, 0, 0, 0, 0)
    assert L.ocean_device_bounds_tiles(b._h, None, None, None, None, None, None) == 0
    b.compute_waves(1.0)
    assert read_code(b, 0) == E_NOT_READY and _patch_code(b) == E_NOT_READY   # a frame, but no set
    for first, count in ((0, 0), (TILES, 1), (0, TILES + 1), (3, 2), (1, 0xFFFFFFFF)):
        assert L.ocean_build_bounds_tiles(b._h, first, count, 1) == E_INVALID, (first, count)
    for first_level in (5, 6, 0xFFFFFFFF):                                  # log2 16 = 4
        assert L.ocean_build_bounds_tiles(b._h, 0, 1, first_level) == E_INVALID, first_level
    assert read_code(b, 0) == E_NOT_READY                                   # (a refused build leaves no set)
    assert L.ocean_build_bounds_tiles(b._h, 1, 2, 4) == 0
    assert read_code(b, 1) == 0 and read_code(b, 2) == 0
    assert read_code(b, 0) == E_NOT_READY and read_code(b, 3) == E_NOT_READY
    assert read_code(b, TILES) == E_INVALID
    assert _patch_code(b, 1, 2) == 0 and _patch_code(b, 0, 2) == E_NOT_READY and _patch_code(b, 2, 2) == E_NOT_READY
    b.compute_waves(2.0)                                                    # a new frame: the query finds the set stale
    assert _patch_code(b, 1, 2) == E_NOT_READY
    assert L.ocean_build_bounds_tiles(b._h, 0, TILES, 0) == 0 and _patch_code(b, 1, 2) == 0
    b.prepare(0x5EED0011)                                                   # the set is gone with the spectrum it came from
    assert read_code(b, 1) == E_NOT_READY and _patch_code(b, 1, 2) == E_NOT_READY
    b.compute_waves(1.0)
    assert read_code(b, 1) == E_NOT_READY and _patch_code(b, 1, 2) == E_NOT_READY
    assert L.ocean_build_bounds_tiles(b._h, 0, TILES, 1) == 0 and read_code(b, 1) == 0 and _patch_code(b, 1, 2) == 0
    b.set_tile_size(32)                                                     # ... and with the tile size
    b.prepare(0x5EED0012)
    b.compute_waves(1.0)
    assert read_code(b, 1) == E_NOT_READY and _patch_code(b, 1, 2) == E_NOT_READY
    assert L.ocean_build_bounds_tiles(b._h, 0, 1, 5) == 0 and L.ocean_build_bounds_tiles(b._h, 0, 1, 6) == E_INVALID     # log2 32 = 5
    disp, _ = b.read_maps()
    check_range(b, 0, TILES, 1, disp)
    b.close()


def test_a_full_block_in_the_second_launch():
    """4096^2: level 6 is 64 x 64, so the second launch takes a whole block from the two chains.  One tile, first_level 4."""
    b = batch(4096, tiles=1)
    b.compute_waves_async(1.25)
    b.build_bounds_tiles(0, 1, 4)
    got = b.read_bounds_tile(0)
    disp, _ = b.read_maps()
    want = B.pyramid(disp[0])
    assert len(got) == 12
    for l in range(4, 13):
        assert same_bits(got[l - 1][0], want[l - 1][0]) and same_bits(got[l - 1][1], want[l - 1][1]), l
    b.close()
