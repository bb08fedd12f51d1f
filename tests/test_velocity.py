"""CPU tests of the water-velocity feature (include/ocean_consumers.h: derivative twin tiles, ocean_query_velocity,
ocean_buoyancy_bodies_flow): the identity the twins rest on, in float64; the float32 restatements of tests/velocity.py against
independent statements of the same rules; the new entry points' argument checks that need no device."""
import ctypes as C

import numpy as np
import pytest

import buoyancy as B
import surface_query as Q
import velocity as V

F = np.float32
DT = 1.0 / 32.0


def prep(n, seed=1234, **kw):
    from oracle import oracle as O
    return O.numpy_prepare(n, O.gauss_xi_numpy(seed, n), **kw)


@pytest.mark.parametrize("n,t", [(16, 0.0), (64, 12.5)])
def test_twin_spectrum_is_the_time_derivative_in_float64(n, t):
    """h(k, t) = h0 e^{i w t} (the animated spectrum is twice its real part) against the twin's h0' e^{i w t}, h0' = i w h0: a central
    difference at +-dt misses the derivative by at most dt^2 / 6 * max |h'''| = w^3 dt^2 / 6 |h0| <= max(w)^2 dt^2 / 6 * |w h0| per bin."""
    p = prep(n)
    h0, w = p["h0"].astype(np.complex128), p["omega"].astype(np.float64)
    twin = 1j * w * h0
    central = (h0 * np.exp(1j * w * (t + DT)) - h0 * np.exp(1j * w * (t - DT))) / (2.0 * DT)
    bound = w.max() ** 2 * DT ** 2 / 6.0 * np.abs(w * h0)
    err = np.abs(twin * np.exp(1j * w * t) - central)
    assert np.abs(twin).max() > 0.0
    assert (err <= bound).all(), float((err - bound).max())
    # the real form the frames evaluate, 2 Re(.), obeys twice the bound
    assert (np.abs(2.0 * (twin * np.exp(1j * w * t)).real - 2.0 * central.real) <= 2.0 * bound).all()


def test_restated_twin_spectrum_is_one_rounding_per_component():
    """derive_spectrum in fp32 = the exact product of two floats (exact in float64) rounded once, sign included; zero bins stay zero."""
    p = prep(64)
    got = V.derive_spectrum(p["h0"], p["omega"])
    w = p["omega"].astype(np.float64)
    want = np.stack([-(w * p["h0"].imag.astype(np.float64)), w * p["h0"].real.astype(np.float64)], axis=-1).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(V.derive_spectrum(np.stack([p["h0"].real, p["h0"].imag], axis=-1), p["omega"]), got)
    assert not got[p["omega"] == 0.0].any()


def test_twin_maps_are_the_time_derivative_of_the_source_maps():
    """numpy_compute_waves on the restated twin spectrum against a central difference of the source's frames, N = 16: every displacement
    channel (the height times its amplitude) and every normal-map channel within the Taylor remainder summed over the spectrum,
    dt^2 / 6 * sum_k w^3 * 2 |h0| * (the channel's weight), plus the float32 rounding of the phases the oracle forms in fp32."""
    from oracle import oracle as O
    n, t = 16, 12.5
    p = prep(n, seed=77)
    tw = dict(p, h0=V.as_complex(V.derive_spectrum(p["h0"], p["omega"])))
    amp, d, q, _, _ = O.numpy_compute_waves(tw, t)
    a0, d0, q0, _, _ = O.numpy_compute_waves(p, t - DT)
    a1, d1, q1, _, _ = O.numpy_compute_waves(p, t + DT)
    w, h0 = p["omega"].astype(np.float64), np.abs(p["h0"].astype(np.complex128))
    kx, kz = np.abs(p["kx"].astype(np.float64)), np.abs(p["kz"].astype(np.float64))
    rem = DT ** 2 / 6.0 * w ** 3 * 2.0 * h0
    # what the oracle rounds to fp32 per bin and frame: the phase w * t (half an ulp of it, 2^-24 w t), then cos / sin, their products with
    # h0 and the difference (4 roundings of 2^-24) -- on 2 |h0|, in both frames of the difference, over 2 dt
    rnd = 2.0 * h0 * 2.0 ** -24 * (w * (t + DT) + 4.0) * 2.0 / (2.0 * DT)
    weights = [np.ones_like(w), np.ones_like(w), np.ones_like(w)], [kx, kz, kx, kz]
    got_d = [d[..., 0], d[..., 1] * amp, d[..., 2]]
    want_d = [(d1[..., 0] - d0[..., 0]) / (2 * DT), (d1[..., 1] * a1 - d0[..., 1] * a0) / (2 * DT), (d1[..., 2] - d0[..., 2]) / (2 * DT)]
    for g, wn, wt in zip(got_d, want_d, weights[0]):
        assert np.abs(g - wn).max() <= ((rem + rnd) * wt).sum(), (np.abs(g - wn).max(), ((rem + rnd) * wt).sum())
        assert np.abs(g).max() > 100.0 * np.abs(g - wn).max()
    for c in range(4):
        g, wn = q[..., c], (q1[..., c] - q0[..., c]) / (2 * DT)
        assert np.abs(g - wn).max() <= ((rem + rnd) * weights[1][c]).sum()
        assert np.abs(g).max() > 100.0 * np.abs(g - wn).max()


def surface(n, seed, lam=-1.0, t=3.7):
    """One source tile and its twin through the float64 oracle, as float32 maps: what a frame would have written."""
    from oracle import oracle as O
    p = prep(n, seed=seed)
    tw = dict(p, h0=V.as_complex(V.derive_spectrum(p["h0"], p["omega"])))
    a, d, q, _, _ = O.numpy_compute_waves(p, t, lam=lam)
    ta, td, _, _, _ = O.numpy_compute_waves(tw, t, lam=lam)
    return (d.astype(np.float32), q.astype(np.float32), F(a)), (td.astype(np.float32), F(ta))


def test_restated_velocity_query():
    """pos is the surface query's, the residual slot is its residual, and V is the twins' displacement sample (the height times A') at the
    rest point of the query's Newton steps, from 0.0f in cascade order."""
    from oracle.consumer import sample_linear_repeat
    n, grid, vd, lam = 16, 512, 1000.0 / 512, -1.0
    (d, q, a), (td, ta) = surface(n, 5, lam)
    xz = np.random.default_rng(3).uniform(-400.0, 400.0, (257, 2)).astype(np.float32)
    for k in (1, 8):
        pos, vel = V.query_velocity([d], [q], [a], [td], [ta], [lam], [1000.0], [1.0], grid, vd, lam, xz, k)
        wpos, wnrm = Q.query_surface([d], [q], [a], [lam], [1000.0], [1.0], grid, vd, lam, xz, k)
        assert np.array_equal(pos.view(np.uint32), wpos.view(np.uint32)) and np.array_equal(vel[:, 3], wnrm[:, 3])
        rx, rz = V.rest_points([d], [q], [a], [lam], [1000.0], [1.0], grid, vd, xz, k)
        u = (rx / F(vd) + F(grid // 2)) / F(grid)
        v = (rz / F(vd) + F(grid // 2)) / F(grid)
        s = sample_linear_repeat(td, u, v)
        want = np.stack([F(0.0) + s[:, 0], F(0.0) + s[:, 1] * ta, F(0.0) + s[:, 2]], axis=1)
        assert np.array_equal(vel[:, :3], want)
        assert np.abs(vel[:, :3]).max() > 0.1
    # two cascades add up in cascade order; a zero twin adds +0.0f
    pos2, vel2 = V.query_velocity([d, d], [q, q], [a, a], [td, np.zeros_like(td)], [ta, ta], [lam, lam], [1000.0, 370.0], [1.0, 2.7], grid, vd, lam, xz, 8)
    rx, rz = V.rest_points([d, d], [q, q], [a, a], [lam, lam], [1000.0, 370.0], [1.0, 2.7], grid, vd, xz, 8)
    assert np.array_equal(vel2[:, :3], V.velocity_at([td], [ta], [1.0], grid, vd, rx, rz))


def test_restated_flow_drag():
    """Still water gives buoyancy.point_terms bit for bit; water that moves with the point leaves Archimedes alone; the drag has the sign
    of the water's velocity for a body at rest."""
    hull = B.box_hull(4, 2, 2, 0.5)
    bodies = B.fleet(5, 0, len(hull), seed=2)
    bi, pi, hi = B.pairs(bodies, len(hull))
    a, p, e = B.world_points(hull, bodies, bi, hi)
    rng = np.random.default_rng(4)
    height = rng.uniform(-1.0, 1.0, len(bi)).astype(np.float32)
    res = rng.uniform(0.0, 1e-3, len(bi)).astype(np.float32)
    weight = F(1025.0) * F(9.81)
    still = V.point_terms_flow(bodies, bi, a, p, e, height, res, np.zeros((len(bi), 3), np.float32), weight, 1000.0)
    assert np.array_equal(still.view(np.uint32), B.point_terms(bodies, bi, a, p, e, height, res, weight, 1000.0).view(np.uint32))
    om = tuple(bodies["omega"][bi, c] for c in range(3))
    oa = B.cross(om, a)
    own = np.stack([bodies["vel"][bi, c] + oa[c] for c in range(3)], axis=1)
    carried = V.point_terms_flow(bodies, bi, a, p, e, height, res, own, weight, 1000.0)
    assert not carried[:, [0, 2]].any() and np.array_equal(carried[:, 1], weight * carried[:, 6])
    rest = B.make_bodies(1)
    rest["points"] = len(hull)
    bi, pi, hi = B.pairs(rest, len(hull))
    water = np.tile(np.array([[1.5, 0.0, -0.5]], np.float32), (len(bi), 1))
    f, tq, _ = V.finish_flow(rest, hull, bi, pi, hi, np.full(len(bi), 10.0, np.float32), np.zeros(len(bi), np.float32), water, 1025.0, 9.81, 1000.0)
    assert f[0, 0] > 0.0 and f[0, 2] < 0.0 and f[0, 3] == F(len(hull) * 0.125)
    assert f[0, 0] == pytest.approx(1000.0 * 1.5 * len(hull) * 0.125, rel=1e-6)


def test_argument_checking_without_device():
    from watersurfacerendering_amd import _abi
    _abi.build()
    L = _abi.lib()
    src = C.c_uint32(7)
    assert _abi.OCEAN_NO_SOURCE == 0xFFFFFFFF
    assert L.ocean_set_velocity_twin(None, 1, 0) == _abi.OCEAN_E_INVALID
    assert L.ocean_velocity_twin(None, 0, C.byref(src)) == _abi.OCEAN_E_INVALID and src.value == 7
    s = _abi.Surface()
    p = _abi.Buoyancy()
    assert L.ocean_query_velocity(None, C.byref(s), None, 0, None, None) == _abi.OCEAN_E_INVALID
    assert L.ocean_query_velocity_device(None, C.byref(s), None, 0, None, None) == _abi.OCEAN_E_INVALID
    assert L.ocean_buoyancy_bodies_flow(None, C.byref(s), C.byref(p), None, 0, None, None) == _abi.OCEAN_E_INVALID
    assert L.ocean_buoyancy_bodies_flow_device(None, C.byref(s), C.byref(p), None, 0, None, None) == _abi.OCEAN_E_INVALID
