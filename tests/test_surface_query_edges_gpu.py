"""The surface query (k_query_surface; solve_rest, eval_surface, clamp_jacobian, sample_linear_repeat) at its edges on the MI355X, bit for
bit.  include/ocean_consumers.h promises fp32 throughout without contraction, the kernels carry `fp contract(off)`, and division and
square root are correctly rounded on both sides, so every comparison here is np.array_equal on the uint32 view of all eight output
floats of every point: no tolerance, no point left out.  The maps are the crafted 16^2 maps of tests/crafted_maps.py, which reach every
branch of the Jacobian clamp; tests/test_surface_query_edges.py asserts on the restatement alone that they do, that every output is finite
and that every texel coordinate stays in the supported range.  Only the last test runs on a Phillips sea."""
import numpy as np
import pytest

import crafted_maps as CM
import surface_query as S

pytestmark = pytest.mark.gpu
F = np.float32
SENTINEL = 0x7FC0BEEF               # a quiet NaN with a payload no result carries
SENTINEL_ROWS = 64


@pytest.fixture(scope="module")
def sea():
    s = CM.Sea()
    yield s
    s.close()


@pytest.fixture(scope="module")
def points():
    return CM.random_points(), CM.special_points()


def _query(sea, xz, first=0, count=1, sc=None, grid=CM.GRID, vd=CM.VD, k=8):
    sc = CM.scales(first, count) if sc is None else sc
    return CM.bits(*sea.b.query_surface(xz, first, sc, grid, vd, CM.CHOPPY, k))


def _query_device(sea, d_xz_ptr, count, cascades, k=8):
    """The device form into outputs of count + SENTINEL_ROWS rows pre-filled with a bit pattern: the bits of the whole allocation."""
    import torch
    d_pos = torch.full((count + SENTINEL_ROWS, 4), SENTINEL, dtype=torch.int32, device="cuda")
    d_nrm = torch.full((count + SENTINEL_ROWS, 4), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sea.b.query_surface_device(d_xz_ptr, count, d_pos.data_ptr(), d_nrm.data_ptr(), 0, CM.scales(0, cascades), CM.GRID, CM.VD, CM.CHOPPY, k)
    sea.b.synchronize()
    return np.concatenate([d_pos.cpu().numpy(), d_nrm.cpu().numpy()], axis=1).view(np.uint32)


@pytest.mark.parametrize("k", CM.KS)
@pytest.mark.parametrize("cascades", [1, 8])
def test_clamp_matrix(sea, points, cascades, k):
    """Kernel == restatement on the crafted maps, one cascade (J takes the block values themselves, exact zeros included) and eight
    (every cascade adds to J), after 1, 2, 3 and 8 Newton steps: on 4099 random points, and on every texel centre and corner of the map,
    also whole mesh periods away, where the texel coordinates are negative."""
    for name, xz in zip(("random", "special"), points):
        assert len(xz) <= CM.POINTS
        got = _query(sea, xz, 0, cascades, k=k)
        want = CM.bits(*sea.restate(0, cascades, CM.scales(0, cascades), CM.GRID, CM.VD, xz, k))
        CM.assert_same_bits(got, want, f"{cascades} cascades K={k} {name} points")


@pytest.mark.parametrize("k", CM.KS)
@pytest.mark.parametrize("cascades", [1, 8])
def test_the_rest_point_itself(sea, points, cascades, k):
    """solve_rest without P in between: the foam query's (rest x, rest z, residual) are the restatement's r_K and residual, bit for bit.
    The velocity and buoyancy kernels take their rest points from the same function."""
    for name, xz in zip(("random", "special"), points):
        out = sea.b.query_foam(xz, 0, CM.scales(0, cascades), CM.GRID, CM.VD, CM.CHOPPY, k)
        _, nr, det = sea.restate(0, cascades, CM.scales(0, cascades), CM.GRID, CM.VD, xz, k, detail=True)
        CM.assert_same_bits(CM.bits(out[:, 1:4]), CM.bits(np.stack([det.rx, det.rz, nr[:, 3]], axis=1)), f"{cascades} cascades K={k} {name} points")


@pytest.mark.parametrize("case", CM.geometries(), ids=lambda c: c[0])
def test_tile_range_and_geometry(sea, points, case):
    """first_tile > 0 with several cascades (gain_c from each tile's own lambda and length), odd grid sizes, one quad, uv_scales that are
    no ratio of lengths: kernel == restatement, and iterations = 0 is iterations = 8."""
    tag, first, count, sc, grid, vd = case
    for name, xz in zip(("random", "special"), points):
        got = _query(sea, xz, first, count, sc, grid, vd, 8)
        want = CM.bits(*sea.restate(first, count, sc, grid, vd, xz, 8))
        CM.assert_same_bits(got, want, f"{tag}, {name} points")
        CM.assert_same_bits(_query(sea, xz, first, count, sc, grid, vd, 0), got, f"{tag}, {name} points, iterations = 0")
    lam = set(CM.LAMBDAS[first:first + count])
    assert count == 1 or len(lam) > 1                       # a gain taken from the wrong tile is another number


@pytest.mark.parametrize("cascades", [1, 8])
def test_tails(sea, points, cascades):
    """Point counts that leave the last wave or the last block partly filled give the first rows of the whole call; the device form
    writes those rows and not one float beyond them, also from points that are only 8-byte aligned; a permutation of the points permutes
    the rows."""
    import torch
    xz = points[0]
    whole = _query(sea, xz, 0, cascades)
    d_xz = torch.from_numpy(xz).cuda()
    d_shifted = torch.zeros(2 + xz.size, dtype=torch.float32, device="cuda")
    d_shifted[2:] = d_xz.reshape(-1)
    assert d_xz.data_ptr() % 16 == 0 and d_shifted.data_ptr() % 16 == 0
    for count in (1, 63, 64, 65, 255, 256, 257, len(xz)):
        CM.assert_same_bits(_query(sea, xz[:count], 0, cascades), whole[:count], f"{count} points")
        for ptr in (d_xz.data_ptr(), d_shifted.data_ptr() + 8):
            got = _query_device(sea, ptr, count, cascades)
            CM.assert_same_bits(got[:count], whole[:count], f"{count} points, device form, xz at {ptr % 16} mod 16")
            assert np.all(got[count:] == np.uint32(SENTINEL)), (count, ptr % 16)
    perm = np.random.default_rng(5).permutation(len(xz))
    CM.assert_same_bits(_query(sea, xz[perm], 0, cascades), whole[perm], "permuted")


def test_points_that_cannot_be_answered_leave_the_others_alone(sea, points):
    """Rows of NaN, +-inf and |x| = 1e15 (beyond 2^31 texels: unspecified rows, include/ocean_consumers.h) among ordinary points: every
    ordinary row has the bits of a call without them, and nothing is written past `points`.  What the bad rows hold is not asserted."""
    import torch
    bad = np.array([[np.nan, 0.0], [0.0, np.nan], [np.inf, 1.0], [1.0, -np.inf], [1e15, 2.0], [3.0, -1e15], [np.nan, np.nan], [-np.inf, np.inf],
                    [-1e15, 1e15]], np.float32)
    good = points[0][:1000]
    where = np.zeros(len(good) + 150, bool)
    where[np.nonzero(np.arange(len(where)) % 7 == 3)[0][:149]] = True      # every wave of the first blocks holds several
    where[-1] = True                                                       # ... and the last row of the call is one
    assert where.sum() == 150 and (~where).sum() == len(good)
    xz = np.empty((len(where), 2), np.float32)
    xz[~where] = good
    xz[where] = bad[np.arange(150) % len(bad)]
    for cascades in (1, 8):
        want = _query(sea, good, 0, cascades)
        with np.errstate(invalid="ignore"):
            CM.assert_same_bits(_query(sea, xz, 0, cascades)[~where], want, f"{cascades} cascades, host form")
        d_xz = torch.from_numpy(xz).cuda()
        got = _query_device(sea, d_xz.data_ptr(), len(xz), cascades)
        CM.assert_same_bits(got[:len(xz)][~where], want, f"{cascades} cascades, device form")
        assert np.all(got[len(xz):] == np.uint32(SENTINEL)), cascades


@pytest.mark.parametrize("k", [1, 8])
def test_a_real_sea(k):
    """One Phillips frame, 64^2, cascades of 1000 / 370 / 93 m, 4099 points: kernel == restatement bit for bit on every point whose
    restatement residual is < 1e-3 m; the rule of tests/test_surface_query_gpu.py::_compare, unchanged, for the rest.  At K = 8 at most
    1 % of the points are outside that bound (tests/test_surface_query_edges.py asserts the same on oracle maps)."""
    import watersurfacerendering_amd as W
    from test_surface_query_gpu import LENGTHS3, _compare
    n = 64
    b = W.OceanBatch(n, len(LENGTHS3), 0)
    for i, L in enumerate(LENGTHS3):
        b.set_params(tile=i, tile_length=L)
    b.prepare(0x5EED0000 + n)
    amps = [float(a) for a in b.compute_waves(3.7)]
    disp, nrm = b.read_maps()
    sc = [LENGTHS3[0] / L for L in LENGTHS3]
    xz = CM.random_points()
    pos, nr = b.query_surface(xz, 0, sc, CM.GRID, CM.VD, -1.0, k)
    opos, onr = S.query_surface(list(disp), list(nrm), amps, [-1.0] * 3, LENGTHS3, sc, CM.GRID, CM.VD, -1.0, xz, k)
    b.close()
    inside = onr[:, 3] < 1e-3
    same = _compare(pos, nr, opos, onr, ("real sea", k))
    print(f"real sea K={k}: {same}/{len(xz)} points bit-identical; {int(inside.sum())} with a restatement residual < 1e-3 m")
    if k == 8:
        assert (~inside).sum() <= 0.01 * len(xz), int((~inside).sum())
    CM.assert_same_bits(CM.bits(pos, nr)[inside], CM.bits(opos, onr)[inside], f"real sea K={k}")
