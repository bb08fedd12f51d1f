"""The vertex stage (k_displace_grid, k_displace_grid_cascades) on the MI355X, bit for bit against oracle/consumer.py, which claims the
same fp32 order: np.array_equal on the uint32 view of every vertex's eight floats, on the crafted 16^2 maps of tests/crafted_maps.py
(their normal map reaches denominators 1 + choppy * ddx of both signs, never 0: tests/test_surface_query_edges.py asserts that every
expected value is finite; tests/test_consumer.py keeps its tolerance-based tests on real frames).  Grids whose vertex count sits around
one and many 256-thread blocks, with odd and even half; 1, 3 and 8 cascades from tile 0 and from tile 3; uv_scales 1, 0.37 and 2.5."""
import ctypes as C

import numpy as np
import pytest

import crafted_maps as CM
from oracle import consumer as O

pytestmark = pytest.mark.gpu
GRIDS, UV_SCALES, CASCADE_SETS, CHOPPY = CM.VERTEX_GRIDS, CM.VERTEX_UV_SCALES, CM.VERTEX_CASCADE_SETS, CM.VERTEX_CHOPPY
SENTINEL = 0x7FC0BEEF


@pytest.fixture(scope="module")
def sea():
    s = CM.Sea()
    yield s
    s.close()


@pytest.mark.parametrize("grid", GRIDS)
def test_displace_grid_is_the_oracle(sea, grid):
    for tile in (0, 3):
        for uv in UV_SCALES:
            got = CM.bits(*sea.b.displace_grid(tile, grid, CM.VD, uv, CHOPPY))
            want = CM.bits(*O.displace_grid(sea.disp[tile], sea.nrm[tile], sea.amps[tile], grid, CM.VD, uv, CHOPPY))
            assert got.shape == ((grid + 1) ** 2, 8)
            CM.assert_same_bits(got, want, f"grid {grid} tile {tile} uv_scale {uv}")


@pytest.mark.parametrize("grid", GRIDS)
def test_displace_grid_cascades_is_the_oracle(sea, grid):
    for first, count in CASCADE_SETS:
        sl = slice(first, first + count)
        for uv in UV_SCALES:
            sc = CM.scales(first, count, uv)
            got = CM.bits(*sea.b.displace_grid_cascades(sc, first, grid, CM.VD, CHOPPY))
            want = CM.bits(*O.displace_grid_cascades(sea.disp[sl], sea.nrm[sl], sea.amps[sl], sc, grid, CM.VD, CHOPPY))
            CM.assert_same_bits(got, want, f"grid {grid} tiles {first}..{first + count - 1} uv_scale {uv}")
            if count == 1:          # one cascade through the cascade call is the plain call
                CM.assert_same_bits(got, CM.bits(*sea.b.displace_grid(first, grid, CM.VD, sc[0], CHOPPY)), f"grid {grid} tile {first} uv_scale {uv}, plain call")


def test_a_smaller_grid_after_a_larger_one(sea):
    """ocean_read_grid returns exactly the (g + 1)^2 rows of the most recent call: the larger grid's buffer stays, its rows do not leak."""
    b = sea.b
    big = CM.bits(*b.displace_grid(0, 255, CM.VD, 1.0, CHOPPY))
    assert big.shape == (256 * 256, 8)
    for call in ("plain", "cascades"):
        if call == "plain":
            small = CM.bits(*b.displace_grid(0, 3, CM.VD, 1.0, CHOPPY))
        else:
            small = CM.bits(*b.displace_grid_cascades(CM.scales(0, 3), 0, 3, CM.VD, CHOPPY))
        assert small.shape == (16, 8)
        pos = np.full((64, 4), SENTINEL, np.uint32)
        nrm = np.full((64, 4), SENTINEL, np.uint32)
        assert b._L.ocean_read_grid(b._h, pos.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p)) == 0
        CM.assert_same_bits(np.concatenate([pos[:16], nrm[:16]], axis=1), small, call)
        assert np.all(pos[16:] == SENTINEL) and np.all(nrm[16:] == SENTINEL), call
        b.displace_grid(0, 255, CM.VD, 1.0, CHOPPY)
    want = CM.bits(*O.displace_grid(sea.disp[0], sea.nrm[0], sea.amps[0], 3, CM.VD, 1.0, CHOPPY))
    CM.assert_same_bits(CM.bits(*b.displace_grid(0, 3, CM.VD, 1.0, CHOPPY)), want, "grid 3 after grid 255")
    CM.assert_same_bits(CM.bits(*b.displace_grid(0, 255, CM.VD, 1.0, CHOPPY)), big, "grid 255 again")
