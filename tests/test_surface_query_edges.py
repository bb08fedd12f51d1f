"""The inputs of tests/test_surface_query_edges_gpu.py on the restatement alone (tests/surface_query.py, tests/crafted_maps.py): the
conditions that keep the GPU comparisons from going vacuous.  Every class of the Jacobian clamp is reached often, every output is finite
(a NaN has no one bit pattern), every texel coordinate stays where the kernel's int conversion and the restatement's int64 agree, and the
clamp and the sampler's wrap below zero are what the header says on values worked out by hand."""
import numpy as np
import pytest

import crafted_maps as CM
import surface_query as S
from oracle.consumer import sample_linear_repeat

F = np.float32
TEXEL_LIMIT = 2.0 ** 30                 # half the supported range |u * s_c * N| < 2^31 (include/ocean_consumers.h)


@pytest.fixture(scope="module")
def crafted():
    return CM.maps()


@pytest.mark.parametrize("cascades", [1, 8])
def test_every_clamp_class_is_reached(crafted, cascades):
    """POINTS random points, K = 8, both axes, all steps: at least 100 evaluations in each of J >= 0.1, 0 < J < 0.1, J == 0, -0.1 < J < 0
    and J <= -0.1.  With eight cascades the noise of cascades 1 .. 7 moves J off an exact 0: that class is exempt there."""
    disp, nrm = crafted
    pos, nr, det = CM.restate(disp, nrm, CM.CPU_AMPS, 0, cascades, CM.scales(0, cascades), CM.GRID, CM.VD, CM.random_points(), 8, detail=True)
    total = det.census.sum(axis=0)
    print(f"cascades={cascades}: " + ", ".join(f"{name}: {int(c)}" for name, c in zip(S.J_CLASSES, total)))
    assert det.census.shape == (8, 5) and det.census.sum() == 8 * 2 * CM.POINTS                  # (no NaN: every J is in a class)
    for name, c in zip(S.J_CLASSES, total):
        if cascades == 8 and name == "J == 0":
            continue
        assert c >= 100, (cascades, name, int(c))
    assert det.census[0, 1:].sum() > 0 and det.census[-1, 1:].sum() > 0                          # at the first step and at the last


def _cases():
    for cascades in (1, 8):
        for k in CM.KS:
            yield f"{cascades} cascades K={k}", 0, cascades, CM.scales(0, cascades), CM.GRID, CM.VD, k
    for tag, first, count, sc, grid, vd in CM.geometries():
        yield tag, first, count, sc, grid, vd, 8


def test_outputs_are_finite_and_texel_coordinates_in_range(crafted):
    """Every call the GPU tests compare with the restatement: all eight outputs and the rest point finite, and no |u * s_c * N| of any
    evaluation at or above 2^30."""
    disp, nrm = crafted
    for xz in (CM.random_points(), CM.special_points()):
        for tag, first, count, sc, grid, vd, k in _cases():
            pos, nr, det = CM.restate(disp, nrm, CM.CPU_AMPS, first, count, sc, grid, vd, xz, k, detail=True)
            assert np.isfinite(pos).all() and np.isfinite(nr).all() and np.isfinite(det.rx).all() and np.isfinite(det.rz).all(), tag
            assert det.texel_range < TEXEL_LIMIT, (tag, det.texel_range)


def test_detail_is_the_same_query(crafted):
    """detail=True changes nothing; r_K is the point P and the residual were evaluated at; iterations = 0 is 8."""
    disp, nrm = crafted
    xz = CM.random_points(500)
    args = (disp, nrm, CM.CPU_AMPS, 0, 8, CM.scales(0, 8), CM.GRID, CM.VD, xz)
    pos, nr = CM.restate(*args, 8)
    dpos, dnr, det = CM.restate(*args, 8, detail=True)
    assert np.array_equal(CM.bits(pos, nr), CM.bits(dpos, dnr))
    assert np.array_equal(CM.bits(*CM.restate(*args, 0)), CM.bits(pos, nr))
    g = S.gains(CM.LAMBDAS, CM.LENGTHS, CM.scales(0, 8), CM.GRID, CM.VD)
    dx, _, dz, *_ = S._eval(list(disp), list(nrm), CM.CPU_AMPS, CM.scales(0, 8), g, CM.GRID, CM.VD, det.rx, det.rz)
    assert np.array_equal(pos[:, 0], det.rx + dx) and np.array_equal(pos[:, 2], det.rz + dz)
    assert g[0] == F(-1.0)                                                                      # the geometry the block values are made for


def test_special_points_sit_on_texel_centres_and_corners():
    """The special points' texel coordinates on tile 0 (s = u * 16 - 0.5 in the kernel's arithmetic) are integers (centres) or
    integers + 0.5 (corners), negative ones included."""
    xz = CM.special_points()
    u = (xz / F(CM.VD) + F(CM.GRID // 2)) / F(CM.GRID)
    s = u * F(CM.N) - F(0.5)
    frac = s - np.floor(s)
    assert set(np.unique(frac).tolist()) == {0.0, 0.5}
    assert (frac == 0.0).all(axis=1).sum() == (frac == 0.5).all(axis=1).sum() == len(xz) // 2
    assert s.min() < -16.0 and s.max() > 5 * 16.0 and (xz < -500.0).any(axis=1).sum() >= len(xz) // 4


def test_clamp_on_hand_written_values():
    """include/ocean_consumers.h: J = sign(J) * 0.1 where |J| < 0.1 (J == 0 -> +0.1), asserted on bits."""
    t = F(0.1)
    below = np.nextafter(t, F(0.0))
    j = np.array([0.05, -0.05, 0.0, -0.0, t, below, -t, -below, 0.5, -0.5, 1.5], np.float32)
    want = np.array([t, -t, t, t, t, t, -t, -t, 0.5, -0.5, 1.5], np.float32)
    assert np.signbit(j[3]) and below < t
    assert np.array_equal(S._clamp(j).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(S.j_census(j), [3, 2, 2, 2, 2])                                    # (+-0 both count as J == 0)


def test_sampler_wraps_below_zero():
    """One texel worked out by hand: n = 4, u = -1/16, v = -9/16.  s = -0.75: floor -1, weight 0.25, columns -1 & 3 = 3 and 0;
    t = -2.75: floor -3, weight 0.25, rows -3 & 3 = 1 and 2.  With tex[y, x, c] = 16 y + 4 x + c every product is exact:
    (28 * 0.75 + 16 * 0.25) * 0.75 + (44 * 0.75 + 32 * 0.25) * 0.25 = 25 * 0.75 + 41 * 0.25 = 29 (+ c)."""
    y, x, c = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    tex = (16 * y + 4 * x + c).astype(np.float32)
    got = sample_linear_repeat(tex, np.array([-1.0 / 16.0], np.float32), np.array([-9.0 / 16.0], np.float32))
    assert np.array_equal(got, np.array([[29.0, 30.0, 31.0, 32.0]], np.float32))
    whole = sample_linear_repeat(tex, np.array([-1.0 / 16.0 + 3.0], np.float32), np.array([-9.0 / 16.0 + 1.0], np.float32))
    assert np.array_equal(whole, got)                                                            # the same texels from above zero


def test_vertex_stage_expectations_are_finite(crafted):
    """tests/test_vertex_stage_edges_gpu.py compares bits: oracle/consumer.py on every one of its cases gives finite numbers only
    (the amplitudes scale pos.y alone)."""
    from oracle import consumer as O
    disp, nrm = crafted
    for grid in CM.VERTEX_GRIDS:
        for uv in CM.VERTEX_UV_SCALES:
            for tile in (0, 3):
                pos, nr = O.displace_grid(disp[tile], nrm[tile], CM.CPU_AMPS[tile], grid, CM.VD, uv, CM.VERTEX_CHOPPY)
                assert np.isfinite(pos).all() and np.isfinite(nr).all(), (grid, uv, tile)
            for first, count in CM.VERTEX_CASCADE_SETS:
                sl = slice(first, first + count)
                pos, nr = O.displace_grid_cascades(disp[sl], nrm[sl], CM.CPU_AMPS[sl], CM.scales(first, count, uv), grid, CM.VD, CM.VERTEX_CHOPPY)
                assert np.isfinite(pos).all() and np.isfinite(nr).all(), (grid, uv, first, count)
    with np.errstate(divide="ignore", invalid="ignore"):            # ... and at the query's choppy a 16-quad grid's would not be
        _, nr = O.displace_grid(disp[0], nrm[0], CM.CPU_AMPS[0], 16, CM.VD, 1.0, CM.CHOPPY)
    assert np.isnan(nr).any()


def test_a_real_sea_mostly_converges():
    """The condition of the real-sea GPU case, on oracle maps: 64^2, cascades of 1000 / 370 / 93 m, 4099 points, K = 8: at most 1 % of
    the points keep a residual of 1e-3 m or more."""
    from test_surface_query import oracle_maps
    lengths = [1000.0, 370.0, 93.0]
    m = [oracle_maps(64, seed=7 + i, length=L) for i, L in enumerate(lengths)]
    sc = [lengths[0] / L for L in lengths]
    _, nr = S.query_surface([x[1] for x in m], [x[2] for x in m], [x[0] for x in m], [-1.0] * 3, lengths, sc, CM.GRID, CM.VD, -1.0,
                            CM.random_points(), 8)
    outside = int((nr[:, 3] >= 1e-3).sum())
    print(f"real sea, oracle maps: {outside} of {CM.POINTS} points with a residual >= 1e-3 m at K = 8")
    assert outside <= 0.01 * CM.POINTS
