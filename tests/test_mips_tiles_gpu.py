"""ocean_build_mips_tiles on the MI355X: the mip chains of a tile range, built in at most two launches, carry exactly the bits of
oracle/consumer.py::mip_chain of the maps the same frame read out and of ocean_build_mips' chain, tile by tile.  Tile sizes 16 (one
launch, a block smaller than 64), 64 (exactly one full block), 128 (four blocks, then a second launch on a 2 x 2 source) and, against
ocean_build_mips only, 4096 (a full 64 x 64 source in the second launch)."""
import ctypes as C

import numpy as np
import pytest

from oracle import consumer as O

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
    d = np.empty((n, 4), np.float32)
    return b._L.ocean_read_mips_tile(b._h, tile, d.ctypes.data_as(C.c_void_p), None)


def check_range(b, first, count, disp, nrm, against_single=True):
    b.build_mips_tiles(first, count)
    for tile in range(first, first + count):
        dl, ql = b.read_mips_tile(tile)
        want = O.mip_chain(disp[tile]) + O.mip_chain(nrm[tile])
        assert len(dl) == len(ql) == b.tile_size.bit_length() - 1
        for l, (got, ref) in enumerate(zip(dl + ql, want)):
            assert same_bits(got, ref), (first, count, tile, l)
    if against_single:              # (ocean_build_mips keeps its own buffers: the set stays)
        for tile in range(first, first + count):
            sd, sq = b.build_mips(tile)
            dl, ql = b.read_mips_tile(tile)
            for l, (got, ref) in enumerate(zip(dl + ql, sd + sq)):
                assert same_bits(got, ref), (first, count, tile, l)


@pytest.mark.parametrize("n", [16, 64, 128])
def test_every_level_of_every_tile_has_the_chains_bits(n):
    b = batch(n)
    b.compute_waves(1.25)
    disp, nrm = b.read_maps()
    for first, count in RANGES:
        check_range(b, first, count, disp, nrm)
        pd, pq = C.c_void_p(), C.c_void_p()
        f, c, lv = C.c_uint32(9), C.c_uint32(9), C.c_uint32(9)
        assert b._L.ocean_device_mips_tiles(b._h, C.byref(pd), C.byref(pq), C.byref(f), C.byref(c), C.byref(lv)) == 0
        assert pd.value and pq.value and (f.value, c.value, lv.value) == (first, count, n.bit_length() - 1)
    b.close()


def test_a_smaller_range_after_a_larger_one():
    b = batch(64)
    b.compute_waves(0.5)
    disp, nrm = b.read_maps()
    check_range(b, 0, 4, disp, nrm, against_single=False)
    check_range(b, 2, 1, disp, nrm, against_single=False)
    for tile in (0, 1, 3):
        assert read_code(b, tile) == E_NOT_READY, tile
    assert read_code(b, 2) == 0
    # both output pointers are optional
    assert b._L.ocean_read_mips_tile(b._h, 2, None, None) == 0
    b.close()


@pytest.mark.parametrize("depth", [2, 3])
def test_the_set_belongs_to_the_most_recent_frame_at_depth(depth):
    b = batch(128, depth=depth)
    for k in range(depth + 1):      # frames in flight on every chain; the last one is the one the set is built from
        b.compute_waves_async(0.5 + 0.75 * k)
    b.build_mips_tiles(0, TILES)
    disp, nrm = b.read_maps()
    for tile in range(TILES):
        dl, ql = b.read_mips_tile(tile)
        for l, (got, ref) in enumerate(zip(dl + ql, O.mip_chain(disp[tile]) + O.mip_chain(nrm[tile]))):
            assert same_bits(got, ref), (depth, tile, l)
    # and again behind one more frame, on the next chain
    b.compute_waves_async(9.0)
    b.build_mips_tiles(1, 2)
    disp2, nrm2 = b.read_maps()
    assert not np.array_equal(disp2[1], disp[1])
    for tile in (1, 2):
        dl, ql = b.read_mips_tile(tile)
        for l, (got, ref) in enumerate(zip(dl + ql, O.mip_chain(disp2[tile]) + O.mip_chain(nrm2[tile]))):
            assert same_bits(got, ref), (depth, tile, l)
    b.close()


def test_error_cases():
    import watersurfacerendering_amd as W
    L = W._abi.lib()
    assert L.ocean_build_mips_tiles(None, 0, 1) == E_INVALID
    assert L.ocean_read_mips_tile(None, 0, None, None) == E_INVALID
    assert L.ocean_device_mips_tiles(None, None, None, None, None, None) == E_INVALID
    b = W.OceanBatch(16, TILES, 0)
    assert L.ocean_build_mips_tiles(b._h, 0, 1) == E_NOT_READY          # no Prepare
    b.prepare(0x5EED0010)
    assert L.ocean_build_mips_tiles(b._h, 0, 1) == E_NOT_READY          # no frame
    assert read_code(b, 0) == E_NOT_READY
    pd = C.c_void_p(1)
    cnt = C.c_uint32(9)
    assert L.ocean_device_mips_tiles(b._h, C.byref(pd), None, None, C.byref(cnt), None) == 0 and pd.value is None and cnt.value == 0
    b.compute_waves(1.0)
    assert read_code(b, 0) == E_NOT_READY                               # a frame, but no set
    for first, count in ((0, 0), (TILES, 1), (0, TILES + 1), (3, 2), (1, 0xFFFFFFFF)):
        assert L.ocean_build_mips_tiles(b._h, first, count) == E_INVALID, (first, count)
    assert L.ocean_build_mips_tiles(b._h, 1, 2) == 0
    assert read_code(b, 1) == 0 and read_code(b, 2) == 0
    assert read_code(b, 0) == E_NOT_READY and read_code(b, 3) == E_NOT_READY
    assert read_code(b, TILES) == E_INVALID
    b.prepare(0x5EED0011)                                               # the set is gone with the spectrum it came from
    assert read_code(b, 1) == E_NOT_READY
    b.compute_waves(1.0)
    assert read_code(b, 1) == E_NOT_READY
    assert L.ocean_build_mips_tiles(b._h, 0, TILES) == 0 and read_code(b, 1) == 0
    b.set_tile_size(32)                                                 # ... and with the tile size
    b.prepare(0x5EED0012)
    b.compute_waves(1.0)
    assert read_code(b, 1) == E_NOT_READY
    disp, nrm = b.read_maps()
    check_range(b, 0, TILES, disp, nrm, against_single=False)
    b.close()


def test_a_full_block_in_the_second_launch():
    """4096^2: level 6 is 64 x 64, so the second launch takes a whole block from a chain.  One tile, against ocean_build_mips' read-out."""
    b = batch(4096, tiles=1)
    b.compute_waves_async(1.25)
    b.build_mips_tiles(0, 1)
    dl, ql = b.read_mips_tile(0)
    sd, sq = b.build_mips(0)
    assert len(dl) == 12
    for l, (got, ref) in enumerate(zip(dl + ql, sd + sq)):
        assert same_bits(got, ref), l
    b.close()
