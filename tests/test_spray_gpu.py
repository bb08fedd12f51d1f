"""ocean_emit_spray / _device (k_spray_count, k_spray_scan, k_spray_scatter) on the MI355X, bit for bit against tests/spray.py:
np.array_equal on the uint32 view of every row of all three arrays and on both counts, host and device form, on the crafted 16^2 maps of
tests/crafted_maps.py behind a FULL7 and a JACOBIAN frame, without and with twins.  The cases are tests/spray.py's, vetted on the CPU by
tests/test_spray.py.  Outputs are prefilled (NaN / 0xffffffff): the rows from `written` on must keep the prefill."""
import ctypes as C

import numpy as np
import pytest

import crafted_maps as CM
import spray as SP

pytestmark = pytest.mark.gpu
E_INVALID, E_NOT_READY, E_UNSUPPORTED = -1, -4, -6
FILL = 0xffffffff


@pytest.fixture(scope="module")
def sea():
    s = SP.Sea(False)
    yield s
    s.close()


@pytest.fixture(scope="module")
def twin_sea():
    s = SP.Sea(True)
    yield s
    s.close()


def prefilled(capacity):
    return (np.full((capacity, 4), np.nan, np.float32), np.full((capacity, 4), np.nan, np.float32), np.full(capacity, FILL, np.uint32))


def compare(got, want, capacity, what):
    """got: (pos, vel, index) of `capacity` prefilled rows and the two counts; want: the restatement's whole list."""
    (pos, vel, index), (total, written) = got
    wpos, wvel, windex = want
    assert (total, written) == (len(windex), min(len(windex), capacity)), (what, total, written, len(windex), capacity)
    CM.assert_same_bits(CM.bits(pos[:written], vel[:written]), CM.bits(wpos[:written], wvel[:written]), what)
    assert np.array_equal(index[:written], windex[:written]), what
    assert np.isnan(pos[written:]).all() and np.isnan(vel[written:]).all() and np.all(index[written:] == FILL), what + ": rows past the list were written"


def host_form(s, case, capacity):
    tag, _, first, count, sc, grid, vd, window, kw = case
    out = prefilled(capacity)
    pos, vel, index, total = s.b.emit_spray(capacity, window, first, sc, grid, vd, out=out, **kw)
    assert pos.base is out[0] or capacity == 0
    return out, (total, len(index))


def device_form(s, case, capacity):
    import torch
    tag, _, first, count, sc, grid, vd, window, kw = case
    rows = max(capacity, 1)
    d_pos = torch.full((2, rows, 4), float("nan"), dtype=torch.float32, device="cuda")
    d_index = torch.full((rows + 2,), -1, dtype=torch.int32, device="cuda")        # [rows] indices, then the two counts
    torch.cuda.synchronize()
    s.b.emit_spray_device(capacity, d_pos[0].data_ptr(), d_pos[1].data_ptr(), d_index.data_ptr(), d_index[rows:].data_ptr(),
                          window, first, sc, grid, vd, **kw)
    s.b.synchronize()
    p = d_pos.cpu().numpy()
    i = d_index.cpu().numpy().view(np.uint32)
    return (p[0][:capacity], p[1][:capacity], i[:capacity]), (int(i[rows]), int(i[rows + 1]))


def want_of(s, case):
    tag, _, first, count, sc, grid, vd, window, kw = case
    return s.restate(first, count, sc, grid, vd, window, **kw)


@pytest.mark.parametrize("mode", SP.MODES)
def test_every_case_host_and_device_form(sea, mode):
    """Window sizes around a wave, a round, C and scan width * C; windows outside the grid; odd grids; the cascade sets; thinning; all
    and none."""
    s = sea.frame(mode)
    for case in SP.cases(mode, False):
        want = want_of(s, case)
        capacity = len(want[2]) + 3
        compare(host_form(s, case, capacity), want, capacity, f"mode {mode}, {case[0]}, host form")
        compare(device_form(s, case, capacity), want, capacity, f"mode {mode}, {case[0]}, device form")


@pytest.mark.parametrize("mode", SP.MODES)
def test_twinned_sets_carry_the_water_velocity(twin_sea, mode):
    s = twin_sea.frame(mode)
    for case in SP.cases(mode, True):
        want = want_of(s, case)
        assert np.any(want[1][:, :3] != 0.0)
        capacity = len(want[2]) + 3
        compare(host_form(s, case, capacity), want, capacity, f"mode {mode}, {case[0]}, host form")
        compare(device_form(s, case, capacity), want, capacity, f"mode {mode}, {case[0]}, device form")
    # the sources alone, in a context where tiles 4 .. 7 are twins: a set that reaches into the twins is only partly twinned
    sf = s.b._surface(2, CM.scales(2, 3), SP.GRID, SP.VD, 0.0, 0)
    p = s.b._spray(sf, SP.WINDOW, {})
    count = (C.c_uint32 * 2)()
    assert s.b._L.ocean_emit_spray(s.b._h, C.byref(sf), C.byref(p), 0, None, None, None, count) == E_INVALID


@pytest.mark.parametrize("mode", SP.MODES)
def test_capacity(sea, mode):
    s = sea.frame(mode)
    small = [c for c in SP.cases(mode, False) if c[0] == f"{SP.CHUNK + 1} vertices"][0]
    want = want_of(s, small)
    total = len(want[2])
    assert total > 2
    for capacity in (0, 1, total - 1, total, total + 1):
        compare(host_form(s, small, capacity), want, capacity, f"mode {mode}, capacity {capacity} of {total}, host form")
        compare(device_form(s, small, capacity), want, capacity, f"mode {mode}, capacity {capacity} of {total}, device form")
    # a capacity that ends exactly where a chunk begins, and one that ends inside that chunk (tests/test_spray.py checks that they do)
    large = SP.cases(mode, False)[len(SP.SIZES) - 1]
    want = want_of(s, large)
    off = SP.chunk_offsets(want[2], large[7][2] * large[7][3])
    k = len(off) // 2
    for capacity in (int(off[k]), int(off[k]) + 1):
        compare(host_form(s, large, capacity), want, capacity, f"mode {mode}, capacity {capacity} at chunk {k}, host form")
        compare(device_form(s, large, capacity), want, capacity, f"mode {mode}, capacity {capacity} at chunk {k}, device form")


@pytest.mark.parametrize("mode", SP.MODES)
@pytest.mark.parametrize("grid,first,count", [(CM.GRID, 0, 3), (255, 3, 3), (16, 0, 8)])
def test_the_whole_grid_is_the_cascade_vertex_stage(sea, mode, grid, first, count):
    """With the whole grid as window and every vertex passing, out_pos.xyz is ocean_displace_grid_cascades' positions.xyz in every bit;
    behind a JACOBIAN frame J is its w."""
    s = sea.frame(mode)
    sc = CM.scales(first, count)
    verts = (grid + 1) ** 2
    positions, _ = s.b.displace_grid_cascades(sc, first, grid, CM.VD, CM.VERTEX_CHOPPY)
    pos, vel, index, total = s.b.emit_spray(verts, None, first, sc, grid, CM.VD, threshold=SP.ALL_PASS)
    assert total == verts and np.array_equal(index, np.arange(verts, dtype=np.uint32))
    assert np.array_equal(pos[:, :3].view(np.uint32), positions[index, :3].view(np.uint32))
    if mode == SP.JACOBIAN:
        assert np.array_equal(vel[:, 3].view(np.uint32), positions[index, 3].view(np.uint32))
    # and thinned to a list: the same rows
    pos, vel, index, total = s.b.emit_spray(verts, None, first, sc, grid, CM.VD, threshold=SP.ALL_PASS, **SP.THIN)
    assert 0 < total < verts and total == len(index)
    assert np.array_equal(pos[:, :3].view(np.uint32), positions[index, :3].view(np.uint32))


def test_two_calls_behind_one_frame_return_identical_bytes(sea):
    import torch
    s = sea.frame(SP.FULL7)
    case = SP.cases(SP.FULL7, False)[len(SP.SIZES) - 1]
    tag, _, first, count, sc, grid, vd, window, kw = case
    total = s.b.emit_spray(0, window, first, sc, grid, vd, **kw)[3]
    runs = []
    for _ in range(2):
        d = torch.zeros((total * 9 + 2,), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s.b.emit_spray_device(total, d.data_ptr(), d[4 * total:].data_ptr(), d[8 * total:].data_ptr(), d[9 * total:].data_ptr(),
                              window, first, sc, grid, vd, **kw)
        s.b.synchronize()
        runs.append(d.cpu().numpy().tobytes())
    assert runs[0] == runs[1] and np.frombuffer(runs[0], np.uint32)[9 * total] == total > 0


def test_errors(sea):
    import watersurfacerendering_amd as W
    s = sea.frame(SP.FULL7)
    b, L = s.b, s.b._L
    count = (C.c_uint32 * 2)(7, 7)
    out = prefilled(4)
    ptr = [a.ctypes.data_as(C.c_void_p) for a in out]

    def call(sf, p, capacity=4, outs=ptr, cnt=count, device=False):
        fn = L.ocean_emit_spray_device if device else L.ocean_emit_spray
        return fn(b._h, C.byref(sf) if sf is not None else None, C.byref(p) if p is not None else None, capacity, outs[0], outs[1], outs[2], cnt)

    def surface(**kw):
        sf = b._surface(0, CM.scales(0, 3), SP.GRID, SP.VD, 0.0, 0)
        for k, v in kw.items():
            setattr(sf, k, v)
        return sf

    def spray(**kw):
        return b._spray(surface(), SP.WINDOW, kw)

    for device in (False, True):
        # the settings
        assert call(surface(), None, device=device) == E_INVALID
        for bad in (dict(nx=0), dict(ny=0), dict(nx=4097, ny=4096), dict(nx=0xffffffff, ny=0xffffffff), dict(thin_log2=17),
                    dict(threshold=float("nan")), dict(threshold=float("inf")), dict(gain=float("nan")), dict(gain=float("-inf")),
                    dict(gain=-0.5), dict(min_rise=float("nan")), dict(min_rise=float("inf"))):
            p = spray()
            for k, v in bad.items():
                setattr(p, k, v)
            assert call(surface(), p, device=device) == E_INVALID, bad
        # the surface: the cases of ocean_query_surface
        assert call(None, spray(), device=device) == E_INVALID
        for bad in (dict(cascades=0), dict(cascades=9), dict(first_tile=CM.TILES), dict(first_tile=6, cascades=3), dict(grid_size=0)):
            assert call(surface(**bad), spray(), device=device) == E_INVALID, bad
        assert (L.ocean_emit_spray_device if device else L.ocean_emit_spray)(None, C.byref(surface()), C.byref(spray()), 0, None, None, None, count) == E_INVALID
        # the pointers: an output only with a capacity, the counts always
        for k in range(3):
            outs = list(ptr)
            outs[k] = None
            assert call(surface(), spray(), outs=outs, device=device) == E_INVALID
        assert call(surface(), spray(), cnt=None, device=device) == E_INVALID
        assert call(surface(), spray(), capacity=0, outs=[None, None, None], cnt=None, device=device) == E_INVALID
    assert list(count) == [7, 7] and np.isnan(out[0]).all() and np.all(out[2] == FILL)
    # capacity 0 does not look at the outputs and still counts; iterations and choppy are not looked at either
    want = s.restate(0, 3, CM.scales(0, 3), SP.GRID, SP.VD, SP.WINDOW)
    assert call(surface(iterations=77, choppy=float("nan")), spray(), capacity=0, outs=[None, None, None]) == 0
    assert list(count) == [len(want[2]), 0]
    # 2^24 vertices are allowed: 16384 chunks, 64 steps of the scan; with every vertex breaking the total is the thinning's alone
    kept = (SP.hash32(np.arange(1 << 24, dtype=np.uint32) + np.uint32(SP.THIN["salt"])) & np.uint32(7)) == 0
    assert b.emit_spray(0, (-2048, -2048, 4096, 4096), 0, CM.scales(0, 3), SP.GRID, SP.VD, threshold=SP.ALL_PASS, **SP.THIN)[3] == int(kept.sum())
    # readiness and the frame's mode
    fresh = W.OceanBatch(CM.N, 2, 0)
    sf, p = fresh._surface(0, [1.0], SP.GRID, SP.VD, 0.0, 0), spray()
    for device in (False, True):
        fn = fresh._L.ocean_emit_spray_device if device else fresh._L.ocean_emit_spray
        assert fn(fresh._h, C.byref(sf), C.byref(p), 0, None, None, None, count) == E_NOT_READY
    fresh.prepare(1)
    assert fresh._L.ocean_emit_spray(fresh._h, C.byref(sf), C.byref(p), 0, None, None, None, count) == E_NOT_READY
    fresh.set_mode(SP.CHOPPY5)
    fresh.compute_waves(1.0)
    for device in (False, True):
        fn = fresh._L.ocean_emit_spray_device if device else fresh._L.ocean_emit_spray
        assert fn(fresh._h, C.byref(sf), C.byref(p), 0, None, None, None, count) == E_UNSUPPORTED
    fresh.set_mode(SP.FULL7)
    fresh.compute_waves(1.0)
    pos, vel, index, total = fresh.emit_spray(16, (0, 0, 4, 4), grid_size=SP.GRID, vertex_distance=SP.VD, threshold=SP.ALL_PASS)
    assert total == 16 and np.array_equal(index, np.arange(16, dtype=np.uint32)) and np.isfinite(pos).all()
    fresh.close()

