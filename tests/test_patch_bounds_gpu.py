"""ocean_patch_bounds (k_patch_bounds) on the MI355X, bit for bit against tests/bounds.py: np.array_equal on the uint32 view of all eight
floats of every rectangle, host and device form, on the crafted 16^2 maps of tests/crafted_maps.py with the bounds set built over the whole
batch.  The inputs are tests/bounds.py's, vetted on the CPU by tests/test_bounds.py (every branch of the level rule, the node rule and the
classification).  And the guarantee on the device: the vertices ocean_displace_grid_cascades writes for a patch lie inside the patch's box
within the slack tests/test_bounds.py derives, e = 2^-21 * sum_c max|texel_c| (times A_c for y)."""
import ctypes as C

import numpy as np
import pytest

import bounds as B
import crafted_maps as CM

pytestmark = pytest.mark.gpu
E_INVALID, E_NOT_READY = -1, -4


@pytest.fixture(scope="module")
def sea():
    s = CM.Sea()
    yield s
    s.close()


def restate(sea, first, count, sc, grid, vd, rects, first_level, pad, planes):
    sl = slice(first, first + count)
    return B.patch_bounds(sea.disp[sl], sea.amps[sl], sc, grid, vd, rects, first_level, pad, planes)


def test_the_set_is_the_pyramid_of_the_crafted_maps(sea):
    """(the maps were written into the bound tensors behind the frame: the set must come from them, not from the Phillips frame)"""
    sea.b.build_bounds_tiles(0, CM.TILES, 1)
    for tile in (0, 5):
        for (glo, ghi), (wlo, whi) in zip(sea.b.read_bounds_tile(tile), B.pyramid(sea.disp[tile])):
            assert np.array_equal(glo.view(np.uint32), wlo.view(np.uint32)) and np.array_equal(ghi.view(np.uint32), whi.view(np.uint32))


@pytest.mark.parametrize("first_level", B.FIRST_LEVELS)
def test_host_and_device_forms_are_the_restatement(sea, first_level):
    import torch
    b = sea.b
    b.build_bounds_tiles(0, CM.TILES, first_level)
    classes = set()
    for k, (tag, first, count, sc, grid, vd, pad, with_planes) in enumerate(B.cases()):
        rects = B.rect_set(grid, vd)
        planes = B.planes_for(grid, vd) if with_planes else None
        what = f"{tag} pad {pad} planes {with_planes} first_level {first_level}"
        want = CM.bits(*restate(sea, first, count, sc, grid, vd, rects, first_level, pad, planes))
        got = CM.bits(*b.patch_bounds(rects, first, sc, grid, vd, planes, pad))
        assert got.shape == (B.RECTS, 8)
        CM.assert_same_bits(got, want, what)
        if with_planes and grid == CM.GRID:
            classes |= set(np.unique(got[:, 7].view(np.float32)).tolist())
        if k % 3 == 0:
            d_in = torch.from_numpy(rects).cuda()
            d_out = torch.full((2, B.RECTS, 4), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            b.patch_bounds_device(d_in.data_ptr(), B.RECTS, d_out[0].data_ptr(), d_out[1].data_ptr(), first, sc, grid, vd, planes, pad)
            b.synchronize()
            CM.assert_same_bits(CM.bits(d_out[0].cpu().numpy(), d_out[1].cpu().numpy()), want, "device form, " + what)
    assert classes == {0.0, 1.0, 2.0}


def test_a_rectangle_outside_the_supported_range_disturbs_no_other_row(sea):
    b = sea.b
    b.build_bounds_tiles(0, CM.TILES, 1)
    sc = CM.scales(0, 3)
    rects = B.rect_set(CM.GRID, CM.VD)
    planes = B.planes_for(CM.GRID, CM.VD)
    clean = CM.bits(*b.patch_bounds(rects, 0, sc, CM.GRID, CM.VD, planes, 1))
    bad = rects.copy()
    bad[B.NAN_ROW] = np.nan
    bad[B.NAN_ROW + 64, 2] = np.inf
    bad[B.NAN_ROW + 300, 1] = -np.inf
    bad[B.RECTS - 1, 0] = 3.0e38
    got = CM.bits(*b.patch_bounds(bad, 0, sc, CM.GRID, CM.VD, planes, 1))
    keep = np.ones(B.RECTS, bool)
    keep[[B.NAN_ROW, B.NAN_ROW + 64, B.NAN_ROW + 300, B.RECTS - 1]] = False
    CM.assert_same_bits(got[keep], clean[keep], "beside rows that are not finite")
    CM.assert_same_bits(clean, CM.bits(*restate(sea, 0, 3, sc, CM.GRID, CM.VD, rects, 1, 1, planes)), "the clean set")


@pytest.mark.parametrize("grid", [15, 16, 17])
@pytest.mark.parametrize("k", [1, 4])
def test_the_vertices_of_a_patch_lie_inside_its_box(sea, grid, k):
    """Patches of k x k quads of the cascade vertex stage's grid: the (k + 1)^2 vertices it writes (fewer quads at the grid's far edge)
    against the box of the patch's rest rectangle.  VD = 1000/512 is exact and so is every vertex's rest position, so the vertex stage's u
    equals the query's and pad_texels = 0 holds."""
    b = sea.b
    b.build_bounds_tiles(0, CM.TILES, 1)
    side, half = grid + 1, grid // 2
    for first, count, base in ((0, 3, 1.0), (0, 8, 2.5), (3, 3, 0.37)):
        sc = CM.scales(first, count, base)
        sl = slice(first, first + count)
        pos, _ = b.displace_grid_cascades(sc, first, grid, CM.VD, CM.VERTEX_CHOPPY)
        pos = pos.reshape(side, side, 4).astype(np.float64)
        starts = list(range(0, grid, k))
        cells = [(xa, ya, min(xa + k, grid), min(ya + k, grid)) for ya in starts for xa in starts]
        rects = np.array([[(xa - half) * CM.VD, (ya - half) * CM.VD, (xb - half) * CM.VD, (yb - half) * CM.VD] for xa, ya, xb, yb in cells], np.float32)
        lo, hi = b.patch_bounds(rects, first, sc, grid, CM.VD)
        CM.assert_same_bits(CM.bits(lo, hi), CM.bits(*restate(sea, first, count, sc, grid, CM.VD, rects, 1, 0, None)), f"grid {grid} k {k}")
        e = B.slack(sea.disp[sl], sea.amps[sl])
        worst = 0.0
        for r, (xa, ya, xb, yb) in enumerate(cells):
            p = pos[ya:yb + 1, xa:xb + 1].reshape(-1, 4)
            worst = max(worst, (p[:, :3] - hi[r, :3]).max(), (lo[r, :3] - p[:, :3]).max(), (lo[r, 3] - p[:, 3]).max())
            assert np.all(p[:, :3] <= hi[r, :3] + e[:3]) and np.all(p[:, :3] >= lo[r, :3] - e[:3]), (grid, k, first, count, r)
            assert np.all(p[:, 3] >= lo[r, 3] - e[3]), (grid, k, first, count, r)
        print(f"grid {grid} k {k} tiles {first}..{first + count - 1}: largest excess over a box {max(worst, 0.0):.3e} (slack {e.tolist()})")


def _code(b, s, q, rects, lo, hi, count=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return b._L.ocean_patch_bounds(b._h, None if s is None else C.byref(s), None if q is None else C.byref(q), p(rects),
                                   len(rects) if count is None else count, p(lo), p(hi))


def test_error_cases(sea):
    import watersurfacerendering_amd as W
    b = sea.b
    b.build_bounds_tiles(0, CM.TILES, 1)
    q = W._abi.PatchQuery()
    q.pad_texels, q.planes = 7, 3
    b._L.ocean_default_patch_query(C.byref(q))
    assert (q.pad_texels, q.planes) == (0, 0) and all(q.plane[k][j] == 0.0 for k in range(6) for j in range(4))
    b._L.ocean_default_patch_query(None)
    rects = B.rect_set(CM.GRID, CM.VD)[:4]
    lo, hi = np.empty((4, 4), np.float32), np.empty((4, 4), np.float32)
    surface = lambda first=0, sc=(1.0, 0.5, 2.0), grid=CM.GRID, iterations=0: b._surface(first, sc, grid, CM.VD, 0.0, iterations)
    s = surface()
    assert _code(b, s, q, rects, lo, hi) == 0
    assert b._L.ocean_patch_bounds(None, C.byref(s), C.byref(q), None, 0, None, None) == E_INVALID
    assert b._L.ocean_patch_bounds_device(None, C.byref(s), C.byref(q), None, 0, None, None) == E_INVALID
    assert _code(b, None, q, rects, lo, hi) == E_INVALID and _code(b, s, None, rects, lo, hi) == E_INVALID
    bad = b._patch_query(None, 65537)
    assert _code(b, s, bad, rects, lo, hi) == E_INVALID and _code(b, s, b._patch_query(None, 65536), rects, lo, hi) == 0
    bad = b._patch_query([[1, 0, 0, 0]] * 6, 0)
    assert _code(b, s, bad, rects, lo, hi) == 0
    bad.planes = 7
    assert _code(b, s, bad, rects, lo, hi) == E_INVALID
    for value in (float("nan"), float("inf"), float("-inf")):
        bad = b._patch_query([[1, 0, 0, 0], [0, value, 0, 0]], 0)
        assert _code(b, s, bad, rects, lo, hi) == E_INVALID, value
        bad.planes = 1                                                      # (only the planes in use are looked at)
        assert _code(b, s, bad, rects, lo, hi) == 0, value
    assert _code(b, s, q, rects, lo, hi, count=0) == 0
    assert _code(b, s, q, None, None, None, count=0) == 0                   # nothing to do: before the pointers are looked at
    assert _code(b, s, q, None, lo, hi, count=4) == E_INVALID
    assert _code(b, s, q, rects, None, hi) == E_INVALID and _code(b, s, q, rects, lo, None) == E_INVALID
    for first, sc in ((CM.TILES, [1.0]), (6, [1.0, 1.0, 1.0])):              # a tile range outside the batch
        assert _code(b, surface(first, sc), q, rects, lo, hi) == E_INVALID
    none = surface(); none.cascades = 0
    many = surface(); many.cascades = 9
    flat = surface(grid=0)
    assert [_code(b, x, q, rects, lo, hi) for x in (none, many, flat)] == [E_INVALID] * 3
    assert _code(b, surface(iterations=77), q, rects, lo, hi) == 0          # iterations are not looked at
    # readiness: a set over another range, then over another frame
    b.build_bounds_tiles(2, 4, 1)                                           # tiles 2 .. 5
    assert _code(b, s, q, rects, lo, hi) == E_NOT_READY and _code(b, surface(3, (1.0, 1.0, 1.0)), q, rects, lo, hi) == 0
    assert _code(b, surface(3, (1.0,) * 4), q, rects, lo, hi) == E_NOT_READY
    assert _code(b, s, q, None, None, None, count=0) == E_NOT_READY         # readiness does not depend on the data
    b.build_bounds_tiles(0, CM.TILES, 1)
    assert _code(b, s, q, rects, lo, hi) == 0
