"""The restatement tests/spray.py of the spray emitters, without a device: it evaluates a vertex as the cascade vertex stage's restatement
does, its hash is the header's, and the cases tests/test_spray_gpu.py runs are what they claim to be -- mixed ones mixed, all-pass and
none-pass exactly that, the thinning and min_rise each keep some breaking vertices and drop others."""
import ctypes as C

import numpy as np
import pytest

import crafted_maps as CM
import spray as SP
from oracle.consumer import displace_grid_cascades

AMPS = list(CM.CPU_AMPS)


@pytest.fixture(scope="module")
def maps():
    return CM.maps()


def run(maps, mode, twinned, case):
    """(breaking, rising, kept, (pos, vel, index)) of one case on the crafted maps."""
    tag, mixed, first, count, sc, grid, vd, window, kw = case
    disp, nrm = maps
    sl, tw = slice(first, first + count), slice(first + 4, first + 4 + count)
    _, j, v = SP.evaluate(list(disp[sl]), list(nrm[sl]), AMPS[sl], CM.LAMBDAS[sl], sc, grid, vd, window, mode == SP.JACOBIAN,
                          list(disp[tw]) if twinned else None, AMPS[tw] if twinned else None)
    terms = SP.predicate(j, v, twinned, SP.params(**kw), window[2] * window[3])
    return terms + (SP.restate(disp, nrm, AMPS, mode, twinned, first, count, sc, grid, vd, window, **kw),)


@pytest.mark.parametrize("grid", [16, 37, 40])
@pytest.mark.parametrize("first,count", SP.CASCADE_SETS)
def test_whole_grid_positions_are_the_vertex_stages(maps, grid, first, count):
    disp, nrm = maps
    sl = slice(first, first + count)
    sc = CM.scales(first, count)
    want, _ = displace_grid_cascades(list(disp[sl]), list(nrm[sl]), AMPS[sl], sc, grid, SP.VD, CM.VERTEX_CHOPPY)
    for mode in SP.MODES:
        pos, vel, index = SP.restate(disp, nrm, AMPS, mode, False, first, count, sc, grid, SP.VD, SP.whole_grid(grid), threshold=SP.ALL_PASS)
        assert np.array_equal(index, np.arange((grid + 1) ** 2, dtype=np.uint32))
        assert np.array_equal(pos[:, :3].view(np.uint32), want[:, :3].view(np.uint32))
        assert not vel[:, :3].any()
        if mode == SP.JACOBIAN:         # J is the vertex stage's w = min_c D_c.w
            assert np.array_equal(vel[:, 3].view(np.uint32), want[:, 3].view(np.uint32))


def test_a_window_is_a_slice_of_the_endless_grid(maps):
    """A window inside the grid lists the whole grid's rows for its vertices; one a whole number of periods away (tile 0 alone at scale 1:
    grid_size vertices) the same J."""
    disp, nrm = maps
    grid, half = SP.GRID, SP.GRID // 2
    whole = SP.restate(disp, nrm, AMPS, SP.FULL7, False, 0, 3, CM.scales(0, 3), grid, SP.VD, SP.whole_grid(grid), threshold=SP.ALL_PASS)
    ix0, iy0, nx, ny = 3, -7, 9, 5
    part = SP.restate(disp, nrm, AMPS, SP.FULL7, False, 0, 3, CM.scales(0, 3), grid, SP.VD, (ix0, iy0, nx, ny), threshold=SP.ALL_PASS)
    i = np.arange(nx * ny)
    rows = (iy0 + i // nx + half) * (grid + 1) + (ix0 + i % nx + half)
    assert np.array_equal(part[0].view(np.uint32), whole[0][rows].view(np.uint32))
    assert np.array_equal(part[1].view(np.uint32), whole[1][rows].view(np.uint32))
    # (grid 16: u = k / 16 + periods is exact in fp32, so the texel weights are the same bits a period away)
    one = SP.restate(disp, nrm, AMPS, SP.FULL7, False, 0, 1, [1.0], 16, 62.5, (ix0, iy0, nx, ny), threshold=SP.ALL_PASS)
    far = SP.restate(disp, nrm, AMPS, SP.FULL7, False, 0, 1, [1.0], 16, 62.5, (ix0 + 3 * 16, iy0 - 2 * 16, nx, ny), threshold=SP.ALL_PASS)
    assert np.array_equal(one[1][:, 3].view(np.uint32), far[1][:, 3].view(np.uint32))


def test_hash_is_the_scalar_one():
    xs = [0, 1, 2, 0x7fffffff, 0x80000000, 0xffffffff, 12345, 0x9E3779B9] + [int(x) for x in np.random.default_rng(5).integers(0, 2 ** 32, 500)]
    got = SP.hash32(np.array(xs, dtype=np.uint32))
    assert got.dtype == np.uint32 and got.tolist() == [SP.hash32_scalar(x) for x in xs]
    assert SP.hash32_scalar(0) == 0 and SP.hash32_scalar(1) != 1
    # i + salt wraps
    assert SP.hash32(np.array([5], np.uint32) + np.uint32(0xfffffffe)).tolist() == [SP.hash32_scalar(3)]
    # the low bits are usable on their own: about one in eight of consecutive indices
    low = (SP.hash32(np.arange(1 << 16, dtype=np.uint32)) & np.uint32(7)) == 0
    assert 0.11 < low.mean() < 0.14


@pytest.mark.parametrize("twinned", [False, True])
@pytest.mark.parametrize("mode", SP.MODES)
def test_the_cases_are_what_they_claim(maps, mode, twinned):
    seen = set()
    for case in SP.cases(mode, twinned):
        tag, mixed, first, count, sc, grid, vd, window, kw = case
        breaking, rising, kept, (pos, vel, index) = run(maps, mode, twinned, case)
        points = window[2] * window[3]
        listed = breaking & rising & kept
        assert np.array_equal(index, np.flatnonzero(listed)) and len(pos) == len(vel) == len(index)
        assert np.all(np.diff(index.astype(np.int64)) > 0)
        if mixed:
            assert listed.sum() >= 64 and points - listed.sum() >= 64, tag
        if tag == "all pass":
            assert listed.all() and len(index) == points
        if tag == "none pass":
            assert not listed.any()
        if kw.get("thin_log2"):
            b = breaking & rising
            assert kw["thin_log2"] == 3 and 0 < listed.sum() < b.sum(), tag
            assert not kept.all() and kept.any()
        if "min_rise" in kw:
            assert twinned and 0 < (breaking & rising).sum() < breaking.sum(), tag
            assert np.all(vel[:, 1] >= np.float32(kw["min_rise"]))
        assert np.all(vel[:, 3] < np.float32(kw["threshold"]))
        assert np.all((pos[:, 3] >= 0.0) & (pos[:, 3] <= 1.0))
        seen.add(tag)
    if not twinned:
        assert {"all pass", "none pass", "thinned"} <= seen
        assert {points for points, _ in SP.SIZES} == {1, 63, 64, 65, 255, 256, 257, SP.CHUNK - 1, SP.CHUNK, SP.CHUNK + 1, SP.SCAN_WIDTH * SP.CHUNK + 1}
        assert (SP.ODD_GRIDS[0] + 1) ** 2 == SP.SCAN_WIDTH * SP.CHUNK
    else:
        assert "min_rise" in seen


def test_chunk_offsets_give_capacities_inside_and_on_a_chunk(maps):
    """What the capacity test on the device relies on: in the largest window some chunk beyond the first starts at a row count that is
    neither 0 nor the total (a capacity that ends exactly on a chunk boundary), and its successor is a capacity that ends inside a chunk."""
    for mode in SP.MODES:
        case = SP.cases(mode, False)[len(SP.SIZES) - 1]
        *_, (pos, vel, index) = run(maps, mode, False, case)
        points = case[7][2] * case[7][3]
        off = SP.chunk_offsets(index, points)
        assert len(off) == SP.SCAN_WIDTH + 1 and off[0] == 0 and np.all(np.diff(off) >= 0)
        k = len(off) // 2
        assert 0 < off[k] < len(index) and off[k] < off[k] + 1 < off[k + 1]
        assert index[off[k]] >= k * SP.CHUNK > index[off[k] - 1]


def test_default_spray():
    from watersurfacerendering_amd import _abi
    p = _abi.Spray()
    p.nx = p.ny = 5
    _abi.lib().ocean_default_spray(C.byref(p))
    assert (p.threshold, p.gain, p.min_rise) == (np.float32(0.3), 2.5, 0.0)
    assert (p.thin_log2, p.salt, p.ix0, p.iy0, p.nx, p.ny) == (0, 0, 0, 0, 0, 0)
    _abi.lib().ocean_default_spray(None)
