"""The LOD sampler (k_sample_surface_lod, k_displace_grid_lod) on the MI355X, bit for bit against tests/lod.py: np.array_equal on the uint32
view of all eight floats of every point or vertex, on the crafted 16^2 maps of tests/crafted_maps.py with the mip set built over the whole
batch.  The inputs are tests/lod.py's, vetted on the CPU by tests/test_lod.py (every branch of the level rule, the undersampled grids
differ from the plain call, every expected value finite)."""
import ctypes as C

import numpy as np
import pytest

import crafted_maps as CM
import lod as L

pytestmark = pytest.mark.gpu
E_INVALID, E_NOT_READY = -1, -4


@pytest.fixture(scope="module")
def sea():
    s = CM.Sea()
    s.b.build_mips_tiles(0, CM.TILES)
    yield s
    s.close()


def restate_points(sea, first, count, base, grid, vd, xzf, scale, max_level):
    sl = slice(first, first + count)
    return L.sample_surface_lod(sea.disp[sl], sea.nrm[sl], sea.amps[sl], CM.scales(first, count, base), grid, vd, L.CHOPPY, xzf, scale, max_level)


def test_the_set_is_the_chain_of_the_crafted_maps(sea):
    """(the maps were written into the bound tensors behind the frame: the set must come from them, not from the Phillips frame)"""
    from oracle import consumer as O
    for tile in (0, 5):
        dl, ql = sea.b.read_mips_tile(tile)
        for got, want in zip(dl + ql, O.mip_chain(sea.disp[tile]) + O.mip_chain(sea.nrm[tile])):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("first,count", L.CASCADE_SETS)
def test_sample_surface_lod_is_the_restatement(sea, first, count):
    ran = 0
    for case in L.point_cases():
        if case[:2] != (first, count):
            continue
        _, _, base, grid, vd, points, scale, max_level = case
        xzf = L.point_set(points, grid, vd)
        keep = L.specified_rows(xzf)
        got = CM.bits(*sea.b.sample_surface_lod(xzf, first, CM.scales(first, count, base), grid, vd, L.CHOPPY, scale, max_level))
        want = CM.bits(*restate_points(sea, first, count, base, grid, vd, xzf, scale, max_level))
        assert got.shape == (points, 8)
        CM.assert_same_bits(got[keep], want[keep], f"tiles {first}..{first + count - 1} uv base {base} grid {grid} points {points} scale {scale} max_level {max_level}")
        # the NaN footprint and the position that is not finite leave every other row as it would be without them
        clean = xzf.copy()
        clean[~keep, 0] = 0.0
        clean[np.isnan(clean[:, 2]), 2] = 0.0
        again = CM.bits(*sea.b.sample_surface_lod(clean, first, CM.scales(first, count, base), grid, vd, L.CHOPPY, scale, max_level))
        CM.assert_same_bits(again[keep], got[keep], "without the NaN footprint and the infinite position")
        ran += 1
    assert ran == len(L.UV_BASES) * len(L.POINT_MESHES)


def test_the_device_form_is_the_host_form(sea):
    import torch
    b = sea.b
    for first, count, base, grid, vd, points, scale, max_level in L.point_cases()[::5]:
        xzf = L.point_set(points, grid, vd)
        sc = CM.scales(first, count, base)
        host = CM.bits(*b.sample_surface_lod(xzf, first, sc, grid, vd, L.CHOPPY, scale, max_level))
        d_in = torch.from_numpy(xzf).cuda()
        d_out = torch.full((2, points, 4), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        b.sample_surface_lod_device(d_in.data_ptr(), points, d_out[0].data_ptr(), d_out[1].data_ptr(), first, sc, grid, vd, L.CHOPPY, scale, max_level)
        b.synchronize()
        dev = CM.bits(d_out[0].cpu().numpy(), d_out[1].cpu().numpy())
        CM.assert_same_bits(dev, host, f"device form, tiles {first}..{first + count - 1} points {points}")


@pytest.mark.parametrize("case", L.GRID_PLAIN, ids=str)
def test_displace_grid_lod_is_the_cascade_call_where_nothing_is_undersampled(sea, case):
    grid, first, count, base, scale, max_level = case
    sl = slice(first, first + count)
    sc = CM.scales(first, count, base)
    got = CM.bits(*sea.b.displace_grid_lod(sc, first, grid, CM.VD, L.CHOPPY, scale, max_level))
    flat = CM.bits(*sea.b.displace_grid_cascades(sc, first, grid, CM.VD, L.CHOPPY))
    want = CM.bits(*L.displace_grid_lod(sea.disp[sl], sea.nrm[sl], sea.amps[sl], sc, grid, CM.VD, L.CHOPPY, scale, max_level))
    assert got.shape == ((grid + 1) ** 2, 8)
    CM.assert_same_bits(got, flat, f"{case}: against ocean_displace_grid_cascades")
    CM.assert_same_bits(got, want, f"{case}: against the restatement")


@pytest.mark.parametrize("case", L.GRID_UNDER, ids=str)
def test_displace_grid_lod_is_the_restatement_where_cascades_are_undersampled(sea, case):
    grid, first, count, base, scale, max_level = case
    sl = slice(first, first + count)
    sc = CM.scales(first, count, base)
    got = CM.bits(*sea.b.displace_grid_lod(sc, first, grid, CM.VD, L.CHOPPY, scale, max_level))
    want = CM.bits(*L.displace_grid_lod(sea.disp[sl], sea.nrm[sl], sea.amps[sl], sc, grid, CM.VD, L.CHOPPY, scale, max_level))
    CM.assert_same_bits(got, want, f"{case}: against the restatement")
    flat = CM.bits(*sea.b.displace_grid_cascades(sc, first, grid, CM.VD, L.CHOPPY))
    differ = (got != flat).any(axis=1)
    assert differ.sum() > len(differ) / 2, (case, int(differ.sum()), len(differ))
    assert np.all(got[:, 7] == 0)           # normals.w = 0.0f


@pytest.mark.parametrize("grid", CM.VERTEX_GRIDS)
def test_the_point_form_at_the_grid_s_rest_points_is_the_cascade_vertex_stage(sea, grid):
    """The two forms that share the cascade sum, held to each other: the point form at footprint 0 on the rest points of the grid the
    vertex stage builds, against ocean_displace_grid_cascades -- words 0 .. 6 of every row, and word 7 = 0 on both sides.  The bits
    match because VD = 125 / 64: xi * VD is exact and x / VD gives xi back, so the point form's (x / vd + half) / grid is the vertex
    stage's (float)(xi + half) / (float)grid, and footprint 0 stays on level 0.  No row is left out."""
    side, half = grid + 1, grid // 2
    i = np.arange(side * side)
    vd = np.float32(CM.VD)
    xzf = np.stack([(i % side - half).astype(np.float32) * vd, (i // side - half).astype(np.float32) * vd,
                    np.zeros(side * side, np.float32)], axis=1)
    for first, count in CM.VERTEX_CASCADE_SETS:
        for base in CM.VERTEX_UV_SCALES:
            sc = CM.scales(first, count, base)
            points = CM.bits(*sea.b.sample_surface_lod(xzf, first, sc, grid, CM.VD, CM.VERTEX_CHOPPY))
            vertices = CM.bits(*sea.b.displace_grid_cascades(sc, first, grid, CM.VD, CM.VERTEX_CHOPPY))
            assert points.shape == vertices.shape == (side * side, 8)
            CM.assert_same_bits(points[:, :7], vertices[:, :7], f"grid {grid} tiles {first}..{first + count - 1} uv base {base}")
            assert not points[:, 7].any() and not vertices[:, 7].any()


def _surface(b, first, scales, grid=CM.GRID, vd=CM.VD, iterations=0):
    return b._surface(first, scales, grid, vd, L.CHOPPY, iterations)


def _point_code(b, s, l, xzf, pos, nrm, points=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return b._L.ocean_sample_surface_lod(b._h, None if s is None else C.byref(s), None if l is None else C.byref(l), p(xzf),
                                         len(xzf) if points is None else points, p(pos), p(nrm))


def _grid_code(b, first, scales, l, grid=16):
    sc = np.ascontiguousarray(scales, dtype=np.float32)
    return b._L.ocean_displace_grid_lod(b._h, first, sc.size, grid, CM.VD, sc.ctypes.data_as(C.POINTER(C.c_float)), L.CHOPPY,
                                        None if l is None else C.byref(l))


def test_error_cases(sea):
    import watersurfacerendering_amd as W
    b = sea.b
    lod = W._abi.Lod()
    b._L.ocean_default_lod(C.byref(lod))
    assert (lod.scale, lod.max_level) == (1.0, 0)
    xzf = L.point_set(4, CM.GRID, CM.VD)
    pos, nrm = np.empty((4, 4), np.float32), np.empty((4, 4), np.float32)
    s = _surface(b, 0, CM.scales(0, 3))
    assert _point_code(b, s, lod, xzf, pos, nrm) == 0
    assert b._L.ocean_sample_surface_lod(None, C.byref(s), C.byref(lod), None, 0, None, None) == E_INVALID
    assert _point_code(b, None, lod, xzf, pos, nrm) == E_INVALID and _point_code(b, s, None, xzf, pos, nrm) == E_INVALID
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        bad = b._lod(scale, 0)
        assert _point_code(b, s, bad, xzf, pos, nrm) == E_INVALID, scale
        assert _grid_code(b, 0, [1.0], bad) == E_INVALID, scale
    assert _point_code(b, s, lod, xzf, pos, nrm, points=0) == 0
    assert _point_code(b, s, lod, None, None, None, points=0) == 0          # nothing to do: before the pointers are looked at
    assert _point_code(b, s, lod, None, pos, nrm, points=4) == E_INVALID
    assert _point_code(b, s, lod, xzf, None, nrm) == E_INVALID and _point_code(b, s, lod, xzf, pos, None) == E_INVALID
    for first, scales in ((CM.TILES, [1.0]), (6, [1.0, 1.0, 1.0])):          # a tile range outside the batch
        assert _point_code(b, _surface(b, first, scales), lod, xzf, pos, nrm) == E_INVALID
    none = _surface(b, 0, [1.0]); none.cascades = 0
    many = _surface(b, 0, [1.0]); many.cascades = 9
    flat = _surface(b, 0, [1.0], grid=0)
    assert [_point_code(b, x, lod, xzf, pos, nrm) for x in (none, many, flat)] == [E_INVALID] * 3
    assert _point_code(b, _surface(b, 0, [1.0], iterations=77), lod, xzf, pos, nrm) == 0      # iterations are ignored
    # the grid form: the cascade call's cases
    assert _grid_code(b, 0, [1.0], lod) == 0 and _grid_code(b, 0, [1.0], None) == E_INVALID
    assert b._L.ocean_displace_grid_lod(None, 0, 1, 16, 1.0, None, -1.0, C.byref(lod)) == E_INVALID
    assert b._L.ocean_displace_grid_lod(b._h, 0, 1, 16, 1.0, None, -1.0, C.byref(lod)) == E_INVALID
    assert _grid_code(b, 0, [1.0] * 9, lod) == E_INVALID and _grid_code(b, 6, [1.0] * 3, lod) == E_INVALID and _grid_code(b, CM.TILES, [1.0], lod) == E_INVALID
    assert _grid_code(b, 0, [1.0], lod, grid=0) == E_INVALID and _grid_code(b, 0, [1.0], lod, grid=8193) == E_INVALID
    assert b._L.ocean_displace_grid_lod(b._h, 0, 0, 16, 1.0, (C.c_float * 1)(1.0), -1.0, C.byref(lod)) == E_INVALID


def test_staleness(sea):
    """A set serves the frame it was built from and the range it was built for: one more frame, another range, ocean_prepare."""
    import torch
    b = sea.b
    lod = b._lod(1.0, 0)
    xzf = L.point_set(256, CM.GRID, CM.VD)
    pos, nrm = np.empty((256, 4), np.float32), np.empty((256, 4), np.float32)
    s = _surface(b, 0, CM.scales(0, 3))
    d_in = torch.from_numpy(xzf).cuda()
    d_out = torch.zeros((2, 256, 4), dtype=torch.float32, device="cuda")

    def codes(surface=s, first=0, scales=CM.scales(0, 3)):
        return (_point_code(b, surface, lod, xzf, pos, nrm),
                b._L.ocean_sample_surface_lod_device(b._h, C.byref(surface), C.byref(lod), C.c_void_p(d_in.data_ptr()), 256,
                                                     C.c_void_p(d_out[0].data_ptr()), C.c_void_p(d_out[1].data_ptr())),
                _grid_code(b, first, scales, lod))

    assert codes() == (0, 0, 0)
    level0 = xzf.copy(); level0[:, 2] = 0.0
    before = CM.bits(*b.sample_surface_lod(xzf, 0, CM.scales(0, 3), CM.GRID, CM.VD, L.CHOPPY))
    try:
        # one more frame -- the Sea's own once more, so that the amplitudes the other tests expect stay; it rewrites the bound tensors, and
        # the crafted maps go back below
        assert [float(a) for a in b.compute_waves(3.7)] == sea.amps
        assert codes() == (E_NOT_READY,) * 3
        assert _point_code(b, s, lod, level0, pos, nrm) == E_NOT_READY          # readiness does not depend on the data
        assert _point_code(b, s, lod, None, None, None, points=0) == E_NOT_READY
        b.synchronize()
        sea.bound.copy_(torch.from_numpy(np.stack([sea.disp, sea.nrm])))
        torch.cuda.synchronize()
        b.build_mips_tiles(2, 4)                        # tiles 2 .. 5
        assert codes() == (E_NOT_READY,) * 3            # tiles 0 .. 2 leave the built range at its lower end
        s35 = _surface(b, 3, CM.scales(3, 3))
        assert codes(s35, 3, CM.scales(3, 3)) == (0, 0, 0)
        s36 = _surface(b, 3, CM.scales(3, 4))
        assert codes(s36, 3, CM.scales(3, 4)) == (E_NOT_READY,) * 3             # ... and at its upper end
        b.build_mips_tiles(0, CM.TILES)
        assert codes() == (0, 0, 0)
        after = CM.bits(*b.sample_surface_lod(xzf, 0, CM.scales(0, 3), CM.GRID, CM.VD, L.CHOPPY))
        keep = L.specified_rows(xzf)
        CM.assert_same_bits(after[keep], before[keep], "the rebuilt set")
    finally:
        b.synchronize()


def test_prepare_drops_the_set():
    """A context of its own: after ocean_prepare the set is gone, with or without a new frame, until it is built again."""
    import watersurfacerendering_amd as W
    b = W.OceanBatch(16, 2, 0)
    b.prepare(1)
    b.compute_waves(1.0)
    lod = b._lod(1.0, 0)
    s = b._surface(0, [1.0, 2.0], 16, 1.0, -1.0, 0)
    xzf = L.point_set(8, 16, 1.0)
    pos, nrm = np.empty((8, 4), np.float32), np.empty((8, 4), np.float32)
    assert _point_code(b, s, lod, xzf, pos, nrm) == E_NOT_READY              # no set yet
    b.build_mips_tiles()
    assert _point_code(b, s, lod, xzf, pos, nrm) == 0 and _grid_code(b, 0, [1.0, 2.0], lod) == 0
    b.prepare(2)
    assert _point_code(b, s, lod, xzf, pos, nrm) == E_NOT_READY and _grid_code(b, 0, [1.0, 2.0], lod) == E_NOT_READY
    b.compute_waves(1.0)
    assert _point_code(b, s, lod, xzf, pos, nrm) == E_NOT_READY and _grid_code(b, 0, [1.0, 2.0], lod) == E_NOT_READY
    b.build_mips_tiles()
    assert _point_code(b, s, lod, xzf, pos, nrm) == 0
    # against the restatement on a real frame's maps, both cascades undersampled on a 4-quad grid
    disp, nrm_maps = b.read_maps()
    amps = [b.heights(i)[0] for i in range(2)]
    got = CM.bits(*b.displace_grid_lod([1.0, 2.0], 0, 4, 1.0, -1.0))
    want = CM.bits(*L.displace_grid_lod(disp, nrm_maps, amps, [1.0, 2.0], 4, 1.0, -1.0))
    CM.assert_same_bits(got, want, "a real frame")
    b.close()
