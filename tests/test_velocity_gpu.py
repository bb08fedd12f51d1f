"""Water velocity on the MI355X (include/ocean_consumers.h: ocean_set_velocity_twin, ocean_query_velocity / _device): the twin spectrum bit
for bit against its float32 restatement, the twins' maps against the float64 oracle run on the restated spectrum, the time derivative
seen through the library (a central difference of the source's frames), the velocity query against tests/velocity.py, and the state and
error rules of the twin table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import surface_query as Q
import velocity as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
F = np.float32
TOL, TOL_AMP = 1e-5, 1e-6               # the suite's parity bounds (tests/test_parity_gpu.py)
GRID = 512
SOURCES = [dict(tile_length=1000.0, anim_period=200.0), dict(tile_length=370.0, anim_period=90.0)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def four_tiles(n, above, seed=11, xi=None, lam=-1.0, **first_source):
    """Two sources of different tile length and animation period and their twins: tiles (2, 3) of (0, 1), or (0, 1) of (2, 3)."""
    import watersurfacerendering_amd as W
    src, tw = ((0, 1), (2, 3)) if above else ((2, 3), (0, 1))
    b = W.OceanBatch(n, 4, 0)
    for s, p in zip(src, SOURCES):
        b.set_params(tile=s, lambda_=lam, **dict(p, **(first_source if s == src[0] else {})))
    for t, s in zip(tw, src):
        b.set_velocity_twin(t, s)
    return b, src, tw


@pytest.mark.parametrize("above", [True, False])
@pytest.mark.parametrize("variant", ["deep", "finite_depth", "capillary", "fp32_omega"])
def test_twin_spectrum_is_the_restatement_bit_for_bit(above, variant):
    b, src, tw = four_tiles(64, above, **(dict(anim_period=1.0e6) if variant == "fp32_omega" else {}))
    if variant == "finite_depth":
        b.set_dispersion(1, 40.0)
    if variant == "capillary":
        b.set_dispersion(2, 5.0)
    b.prepare(0x5EED)
    for s, t in zip(src, tw):
        h0, om = b.read_spectrum(s)
        th0, tom = b.read_spectrum(t)
        assert np.abs(h0).max() > 0.0 and om.max() > 0.0
        assert np.array_equal(bits(tom), bits(om))
        assert np.array_equal(bits(th0), bits(V.derive_spectrum(h0, om))), (variant, above, s, t)
        assert np.array_equal(bits(b.read_xi(t)), bits(b.read_xi(s)))
        ps, pt = b.get_params(s), b.get_params(t)
        assert (ps.tile_length, ps.anim_period, ps.lambda_) == (pt.tile_length, pt.anim_period, pt.lambda_)
    if variant == "fp32_omega":         # the multiples of the base frequency exceed 16 bits: the frames read the fp32 array
        _, om = b.read_spectrum(src[0])
        assert float(om.max()) / (2.0 * np.pi / 1.0e6) > 65536.0
        from watersurfacerendering_amd import _abi
        b.compute_waves(1.0)
        assert b.last_launch()[0]["flags"] & _abi.OCEAN_LAUNCH_FP32_DISPERSION
    assert not np.array_equal(b.read_spectrum(src[0])[1], b.read_spectrum(src[1])[1])
    b.close()


def oracle_pair(n, xi, t, lam, mode, length=1000.0, anim_period=200.0, dispersion=(0, 0.0)):
    """(amp, disp, nrm) of a source and of its twin from the float64 oracle: the twin is numpy_compute_waves on numpy_prepare's
    dictionary with h0 replaced by the restated twin spectrum; the reduced modes drop what the library drops."""
    from oracle import oracle as O
    from watersurfacerendering_amd import _abi
    p = O.numpy_prepare(n, xi, length=length, anim_period=anim_period, dispersion=dispersion)
    tw = dict(p, h0=V.as_complex(V.derive_spectrum(p["h0"], p["omega"])))
    out = []
    for prep in (p, tw):
        a, d, q, _, _ = O.numpy_compute_waves(prep, t, lam=lam, jacobian=mode == _abi.OCEAN_MODE_JACOBIAN)
        if mode == _abi.OCEAN_MODE_CHOPPY5:
            q[..., 2:] = 0.0
        if mode == _abi.OCEAN_MODE_HEIGHT1:
            d[..., [0, 2]] = 0.0
            q[...] = 0.0
        out.append((a, d, q))
    return out


def check_maps(got_amp, got_d, got_q, want, tag):
    a, d, q = want
    print(tag, "amp", got_amp, a)
    assert abs(got_amp - a) <= TOL_AMP * abs(a), (tag, got_amp, a)
    for name, got, ref in (("disp", got_d, d), ("nrm", got_q, q)):
        for c in range(4):
            m = float(np.abs(ref[..., c]).max())
            err = float(np.abs(got[..., c].astype(np.float64) - ref[..., c]).max())
            print(tag, name, c, "max|ref|", m, "err/max", err / max(m, 1e-30))
            if m == 0.0:
                assert np.all(got[..., c] == 0.0), (tag, name, c)
            else:
                assert err <= TOL * m, (tag, name, c, err / m)


@pytest.mark.parametrize("n", [16, 64])
def test_twin_maps_match_the_float64_restatement(n):
    """All four modes, t = 0 and t = 2.25, injected draws (the twin's own part of the array is NaN: it is ignored)."""
    import watersurfacerendering_amd as W
    from oracle import oracle as O
    from watersurfacerendering_amd import _abi
    xi = O.gauss_xi_numpy(4242, n)
    b = W.OceanBatch(n, 2, 0)
    b.set_velocity_twin(0, 1)           # the twin below its source
    b.set_params(tile=1, lambda_=-1.5)
    b.prepare(0, np.stack([np.full_like(xi, np.nan), xi]))
    assert np.array_equal(bits(b.read_xi(0)), bits(xi))
    for mode in (_abi.OCEAN_MODE_FULL7, _abi.OCEAN_MODE_CHOPPY5, _abi.OCEAN_MODE_HEIGHT1, _abi.OCEAN_MODE_JACOBIAN):
        b.set_mode(mode)
        for t in (0.0, 2.25):
            amps = b.compute_waves(t)
            d, q = b.read_maps()
            src, tw = oracle_pair(n, xi, t, -1.5, mode)
            check_maps(float(amps[1]), d[1], q[1], src, (n, mode, t, "source"))
            check_maps(float(amps[0]), d[0], q[0], tw, (n, mode, t, "twin"))
            assert b.heights(0)[0] == amps[0]
    b.close()


def test_fp16_spectrum_twin_maps_within_that_variants_tolerance():
    """ocean_set_spectrum_precision(16): the half2 copy is made from the twin's final spectrum (k_derive_spectrum runs before it), so the
    twin's maps keep the tolerance tests/test_parity_gpu.py states for that variant (FP16_TOL), 1e-3 of each channel's maximum."""
    import watersurfacerendering_amd as W
    from oracle import oracle as O
    from watersurfacerendering_amd import _abi
    n = 64
    xi = O.gauss_xi_numpy(99, n)
    b = W.OceanBatch(n, 2, 0)
    b.set_spectrum_precision(16)
    b.set_velocity_twin(1, 0)
    b.prepare(0, np.stack([xi, xi]))
    amps = b.compute_waves(2.25)
    d, q = b.read_maps()
    _, (a, wd, wq) = oracle_pair(n, xi, 2.25, -1.0, _abi.OCEAN_MODE_FULL7)
    assert abs(float(amps[1]) - a) <= 1e-3 * a
    for got, ref in ((d[1], wd), (q[1], wq)):
        for c in range(4):
            m = float(np.abs(ref[..., c]).max())
            assert float(np.abs(got[..., c] - ref[..., c]).max()) <= 1e-3 * m, c
    b.close()


def test_lambda_and_time_offsets_follow_the_source():
    import watersurfacerendering_amd as W
    from oracle import oracle as O
    from watersurfacerendering_amd import _abi
    n, t = 16, 1.5
    b, src, tw = four_tiles(n, True)
    xi = [O.gauss_xi_numpy(7 + i, n) for i in range(2)]
    b.prepare(0, np.stack(xi + xi))

    def frame(time, lams, offs):
        amps = b.compute_waves(time)
        d, q = b.read_maps()
        for k in range(2):
            p = SOURCES[k]
            s, w = oracle_pair(n, xi[k], time + offs[k], lams[k], _abi.OCEAN_MODE_FULL7, p["tile_length"], p["anim_period"])
            check_maps(float(amps[src[k]]), d[src[k]], q[src[k]], s, ("source", k, lams, offs))
            check_maps(float(amps[tw[k]]), d[tw[k]], q[tw[k]], w, ("twin", k, lams, offs))
        return d

    d0 = frame(t, (-1.0, -1.0), (0.0, 0.0))
    b.set_lambda(-0.5, tile=1)          # per-tile lambdas from now on: the twin of tile 1 takes its source's
    d1 = frame(t, (-1.0, -0.5), (0.0, 0.0))
    assert np.array_equal(bits(d1[2]), bits(d0[2]))
    assert np.allclose(d1[3][..., [0, 2]], 0.5 * d0[3][..., [0, 2]], rtol=1e-6, atol=0) and np.array_equal(bits(d1[3][..., 1]), bits(d0[3][..., 1]))
    for twin in tw:
        with pytest.raises(W.OceanError) as e:
            b.set_lambda(-2.0, tile=twin)
        assert e.value.code == _abi.OCEAN_E_INVALID
        with pytest.raises(W.OceanError) as e:
            b.set_params(tile=twin, wind_speed=3.0)
        assert e.value.code == _abi.OCEAN_E_INVALID
    b.set_lambda(-1.0)                  # OCEAN_ALL_TILES behaves as always
    frame(t, (-1.0, -1.0), (0.0, 0.0))
    b.set_time_offsets([0.25, 4.0, 100.0, -100.0])      # (the twins' own entries are not used)
    frame(t, (-1.0, -1.0), (0.25, 4.0))
    b.set_time_offsets(None)
    frame(t, (-1.0, -1.0), (0.0, 0.0))
    b.close()


def test_the_twin_is_the_central_difference_of_its_sources_frames():
    """N = 64, dt = 1/32: |twin(t) - (source(t + dt) - source(t - dt)) / (2 dt)| per channel <= the Taylor remainder summed over the spectrum in
    float64, dt^2 / 6 * sum_k w^3 * 2 |h0| * (the channel's weight in k), plus 2 * (1e-5 max|channel|) / (2 dt) for the parity error of the
    two frames.  Everything through the library: Prepare with generated draws, three frames, read back."""
    import watersurfacerendering_amd as W
    n, t, dt = 64, 12.5, 1.0 / 32.0
    b = W.OceanBatch(n, 2, 0)
    b.set_velocity_twin(1, 0)
    b.prepare(321)
    h0, om = b.read_spectrum(0)
    a0 = b.compute_waves(t - dt)
    d0, q0 = b.read_maps(0, 1)
    a1 = b.compute_waves(t + dt)
    d1, q1 = b.read_maps(0, 1)
    at = b.compute_waves(t)
    dt_, qt = b.read_maps(1, 1)
    d0, q0, d1, q1, dtw, qtw = (x[0].astype(np.float64) for x in (d0, q0, d1, q1, dt_, qt))
    w = om.astype(np.float64)
    mag = 2.0 * np.hypot(h0[..., 0].astype(np.float64), h0[..., 1].astype(np.float64))
    k1 = np.pi * (2.0 * np.arange(n) - n) / 1000.0
    kx, kz = np.abs(np.broadcast_to(k1[None, :], (n, n))), np.abs(np.broadcast_to(k1[:, None], (n, n)))
    rem = dt ** 2 / 6.0 * w ** 3 * mag
    one = np.ones_like(w)
    cases = [("disp.x", dtw[..., 0], d0[..., 0], d1[..., 0], one), ("height", dtw[..., 1] * float(at[1]), d0[..., 1] * float(a0[0]), d1[..., 1] * float(a1[0]), one),
             ("disp.z", dtw[..., 2], d0[..., 2], d1[..., 2], one)]
    cases += [("nrm.%d" % c, qtw[..., c], q0[..., c], q1[..., c], (kx, kz, kx, kz)[c]) for c in range(4)]
    for name, twin, lo, hi, weight in cases:
        central = (hi - lo) / (2.0 * dt)
        err = float(np.abs(twin - central).max())
        bound = float((rem * weight).sum()) + 2.0 * (TOL * max(float(np.abs(lo).max()), float(np.abs(hi).max()))) / (2.0 * dt)
        print(f"{name}: max|twin| {np.abs(twin).max():.4g}  |twin - central| {err:.3g}  remainder {float((rem * weight).sum()):.3g}  bound {bound:.3g}")
        assert np.abs(twin).max() > 0.0 and err <= bound, (name, err, bound)
    b.close()


def sea(n, cascades, seed=0x5EED, t=3.7, lam=-1.0, twins_first=False, **params):
    """`cascades` sources and their twins in one batch, one FULL7 frame on it."""
    import watersurfacerendering_amd as W
    lengths = [1000.0, 370.0][:cascades]
    b = W.OceanBatch(n, 2 * cascades, 0)
    first = cascades if twins_first else 0
    for i, L in enumerate(lengths):
        b.set_params(tile=first + i, tile_length=L, lambda_=lam, **params)
        b.set_velocity_twin((0 if twins_first else cascades) + i, first + i)
    b.prepare(seed)
    b.compute_waves(t)
    return b, first, (0 if twins_first else cascades), lengths


@pytest.mark.parametrize("cascades", [1, 2])
def test_velocity_query_against_the_restatement(cascades):
    """Points 1, 63, 64, 65, 257; K = 1 and 8; uv_scales (1, 2.7).  out_pos and the residual are ocean_query_surface's, bit for bit; V is the
    restated sample of the twins' maps (read back from the same frame, A' from the twins' keys) at the rest point the library's own foam
    query reports, bit for bit; the device form is the host form.  Against the pure restatement (its own Newton steps) the rule of
    tests/test_surface_query_gpu.py: 1e-5 of each channel's magnitude wherever both residuals are < 1e-3 m."""
    import torch
    for twins_first in (False, True):
        b, first, tfirst, lengths = sea(64, cascades, twins_first=twins_first)
        scales, vd, lam = [1.0, 2.7][:cascades], 1000.0 / GRID, -1.0
        d, q = b.read_maps()
        amps = [b.heights(first + c)[0] for c in range(cascades)]
        tamps = [b.heights(tfirst + c)[0] for c in range(cascades)]
        src_d, src_q = [d[first + c] for c in range(cascades)], [q[first + c] for c in range(cascades)]
        tw_d = [d[tfirst + c] for c in range(cascades)]
        b.update_foam(0.1)              # (only for the rest points the foam query hands out)
        rng = np.random.default_rng(cascades)
        for points in (1, 63, 64, 65, 257):
            xz = rng.uniform(-700.0, 700.0, (points, 2)).astype(np.float32)
            for k in (1, 8):
                geo = dict(first_tile=first, uv_scales=scales, grid_size=GRID, vertex_distance=vd, choppy=lam, iterations=k)
                pos, vel = b.query_velocity(xz, **geo)
                spos, snrm = b.query_surface(xz, **geo)
                assert np.array_equal(bits(pos), bits(spos)) and np.array_equal(bits(vel[:, 3]), bits(snrm[:, 3]))
                rest = b.query_foam(xz, **geo)
                want = V.velocity_at(tw_d, tamps, scales, GRID, vd, rest[:, 1].copy(), rest[:, 2].copy())
                same = (bits(vel[:, :3]) == bits(want)).all(1)
                print(f"cascades={cascades} points={points} K={k}: {int(same.sum())}/{points} velocities bit-identical behind the library's rest point; max|V| {np.abs(vel[:, :3]).max():.3g}")
                assert same.all(), np.nonzero(~same)[0][:8]
                d_xz = torch.from_numpy(xz).cuda()
                d_pos = torch.full((points, 4), float("nan"), dtype=torch.float32, device="cuda")
                d_vel = torch.full_like(d_pos, float("nan"))
                torch.cuda.synchronize()
                b.query_velocity_device(d_xz.data_ptr(), points, d_pos.data_ptr(), d_vel.data_ptr(), **geo)
                b.synchronize()
                assert np.array_equal(bits(d_pos.cpu().numpy()), bits(pos)) and np.array_equal(bits(d_vel.cpu().numpy()), bits(vel))
                if points == 257:
                    opos, ovel = V.query_velocity(src_d, src_q, amps, tw_d, tamps, [lam] * cascades, lengths, scales, GRID, vd, lam, xz, k)
                    scale = np.maximum(np.abs(ovel[:, :3]).max(0), 1e-30)
                    close = np.all(np.abs(vel[:, :3] - ovel[:, :3]) <= 1e-5 * scale, axis=1)
                    both = (vel[:, 3] < 1e-3) & (ovel[:, 3] < 1e-3)
                    print(f"  pure restatement: {int(close.sum())}/{points} within 1e-5, {int(both.sum())} with both residuals < 1e-3 m")
                    assert close[both].all() and (k == 1 or both.any())
        b.close()


def test_a_flat_sea_does_not_move():
    b, first, tfirst, _ = sea(16, 1, phillips_const=0.0)
    xz = np.random.default_rng(0).uniform(-500.0, 500.0, (65, 2)).astype(np.float32)
    pos, vel = b.query_velocity(xz, first_tile=first, grid_size=GRID, vertex_distance=1000.0 / GRID)
    assert not bits(vel).any()                                          # +0.0f in V and in the residual
    assert np.array_equal(pos[:, [0, 2]], xz) and not pos[:, 1].any()
    b.close()


def test_twin_table_state_and_errors():
    import watersurfacerendering_amd as W
    A = W._abi
    n = 16
    b = W.OceanBatch(n, 4, 0)
    L = b._L
    src = C.c_uint32()
    for tile, source in ((4, 0), (0, 4), (1, 1), (0xFFFFFFFF, 0)):      # outside the batch, tile == source
        assert L.ocean_set_velocity_twin(b._h, tile, source) == A.OCEAN_E_INVALID, (tile, source)
    assert L.ocean_velocity_twin(b._h, 4, C.byref(src)) == A.OCEAN_E_INVALID and L.ocean_velocity_twin(b._h, 0, None) == A.OCEAN_E_INVALID
    assert [b.velocity_twin(i) for i in range(4)] == [None] * 4
    b.prepare(1)
    b.compute_waves(0.5)
    plain_d, plain_q = b.read_maps()
    b.set_velocity_twin(2, 0)
    # host state only, but the context is not prepared until the next ocean_prepare
    for call in (lambda: b.compute_waves(0.5), lambda: b.compute_waves_async(0.5), lambda: b.read_maps(), lambda: b.heights(0),
                 lambda: b.query_surface(np.zeros((1, 2), np.float32)), lambda: b.query_velocity(np.zeros((1, 2), np.float32)), lambda: b.read_spectrum(0)):
        with pytest.raises(W.OceanError) as e:
            call()
        assert e.value.code == A.OCEAN_E_NOT_READY
    assert b.velocity_twin(2) == 0 and b.velocity_twin(0) is None
    for tile, source in ((3, 2),        # a source that is itself a twin
                         (0, 1),        # a tile that is some twin's source
                         (3, 0),        # a source that already has another twin
                         (1, 2)):
        assert L.ocean_set_velocity_twin(b._h, tile, source) == A.OCEAN_E_INVALID, (tile, source)
    b.set_velocity_twin(2, 0)           # saying it again is allowed
    b.set_velocity_twin(3, 1)
    b.prepare(1)
    xz = np.random.default_rng(1).uniform(-300.0, 300.0, (64, 2)).astype(np.float32)
    geo = dict(grid_size=GRID, vertex_distance=1000.0 / GRID)
    with pytest.raises(W.OceanError) as e:
        b.query_velocity(xz, **geo)
    assert e.value.code == A.OCEAN_E_NOT_READY                           # prepared, no frame yet
    b.compute_waves(0.5)
    d, q = b.read_maps()
    assert np.array_equal(bits(d[:2]), bits(plain_d[:2])) and np.array_equal(bits(q[:2]), bits(plain_q[:2]))      # the sources are what they were
    assert not np.array_equal(bits(d[2]), bits(plain_d[2]))
    want = b.query_velocity(xz, first_tile=0, uv_scales=(1.0, 2.7), **geo)
    assert np.abs(want[1][:, :3]).max() > 0.0
    b.query_velocity(xz, first_tile=1, **geo)                           # tile 1 alone: its twin is tile 3
    for kw, code in ((dict(first_tile=2), A.OCEAN_E_NOT_READY),         # a set of twins: none of them has a twin
                     (dict(first_tile=1, uv_scales=(1.0, 1.0)), A.OCEAN_E_INVALID),      # tile 1 has a twin, tile 2 has none
                     (dict(first_tile=0, uv_scales=(1.0,) * 3), A.OCEAN_E_INVALID),
                     (dict(first_tile=4), A.OCEAN_E_INVALID), (dict(first_tile=0, uv_scales=(1.0,) * 5), A.OCEAN_E_INVALID),
                     (dict(grid_size=0, vertex_distance=1.0), A.OCEAN_E_INVALID), (dict(iterations=33), A.OCEAN_E_INVALID)):
        with pytest.raises(W.OceanError) as e:
            b.query_velocity(xz, **dict(geo, **kw))
        assert e.value.code == code, kw
    s = b._surface(0, (1.0,), GRID, 1000.0 / GRID, -1.0, 8)
    out = np.zeros((2, 64, 4), np.float32)
    o0, o1, p = out[0].ctypes.data_as(C.c_void_p), out[1].ctypes.data_as(C.c_void_p), xz.ctypes.data_as(C.c_void_p)
    assert L.ocean_query_velocity(b._h, None, p, 64, o0, o1) == A.OCEAN_E_INVALID
    assert L.ocean_query_velocity(b._h, C.byref(s), None, 64, o0, o1) == A.OCEAN_E_INVALID
    assert L.ocean_query_velocity(b._h, C.byref(s), p, 64, None, o1) == A.OCEAN_E_INVALID
    assert L.ocean_query_velocity(b._h, C.byref(s), p, 64, o0, None) == A.OCEAN_E_INVALID
    assert L.ocean_query_velocity_device(b._h, C.byref(s), None, 64, None, None) == A.OCEAN_E_INVALID
    assert L.ocean_query_velocity(b._h, C.byref(s), None, 0, None, None) == A.OCEAN_OK
    assert L.ocean_query_velocity_device(b._h, C.byref(s), None, 0, None, None) == A.OCEAN_OK
    # twins that are not consecutive in cascade order: (3, 2) of (0, 1)
    b.set_velocity_twin(2, None)
    b.set_velocity_twin(3, None)
    b.set_velocity_twin(3, 0)
    b.set_velocity_twin(2, 1)
    b.prepare(1)
    b.compute_waves(0.5)
    with pytest.raises(W.OceanError) as e:
        b.query_velocity(xz, first_tile=0, uv_scales=(1.0, 2.7), **geo)
    assert e.value.code == A.OCEAN_E_INVALID
    b.query_velocity(xz, first_tile=0, **geo)
    # the table survives a new tile size ...
    b.set_tile_size(32)
    assert [b.velocity_twin(i) for i in range(4)] == [None, None, 1, 0]
    b.prepare(1)
    b.compute_waves(0.5)
    h0, om = b.read_spectrum(0)
    assert np.array_equal(bits(b.read_spectrum(3)[0]), bits(V.derive_spectrum(h0, om)))
    b.set_tile_size(n)
    # ... and a tile that is given back is an ordinary tile again: the maps of a context that never had twins
    b.set_velocity_twin(2, None)
    b.set_velocity_twin(3, None)
    b.prepare(1)
    b.compute_waves(0.5)
    d, q = b.read_maps()
    assert np.array_equal(bits(d), bits(plain_d)) and np.array_equal(bits(q), bits(plain_q))
    with pytest.raises(W.OceanError) as e:
        b.query_velocity(xz, **geo)
    assert e.value.code == A.OCEAN_E_NOT_READY                           # no tile of the set has a twin
    b.close()


def test_cpp_adaptor_velocity_matches_python_binding(tmp_path):
    import watersurfacerendering_amd as W
    from watersurfacerendering_amd import _abi
    exe = tmp_path / "velocity_demo"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "velocity_demo.cpp"), "-o", str(exe),
                    "-L", os.path.dirname(_abi.LIB_PATH), "-locean_hip", "-Wl,-rpath," + os.path.dirname(_abi.LIB_PATH),
                    "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = tmp_path / "velocity.bin"
    r = subprocess.run([str(exe), "64", str(out), "3.7"], capture_output=True, text=True, check=True)
    n, amp, count, moving = r.stdout.split()
    count = int(count)
    raw = np.fromfile(out, dtype=np.float32)
    xz = raw[:2 * count].reshape(count, 2)
    cpos = raw[2 * count:6 * count].reshape(count, 4)
    cvel = raw[6 * count:].reshape(count, 4)
    ws = W.WSTessendorf(64, 1000.0, velocity=True)
    ws.SetWindDirection((1.0, 0.5)); ws.SetWindSpeed(20.0); ws.SetLambda(-1.5)
    ws.Prepare(seed=42)
    assert ws.ComputeWaves(3.7) == pytest.approx(float(amp), rel=1e-7)
    pos, vel = ws.QueryVelocity(xz)
    assert np.array_equal(bits(pos), bits(cpos)) and np.array_equal(bits(vel), bits(cvel))
    assert np.array_equal(bits(pos), bits(ws.QuerySurface(xz)[0]))
    assert int(moving) == int((np.abs(vel[:, :3]).max(1) > 0.05).sum()) > count // 2


def test_adaptor_async_pair_with_velocity_returns_the_models_own_tile():
    """ComputeWavesAsync + Wait on a velocity=True model: the back pair holds one tile, so the copy must ask for the model's own tile only
    (the twin's maps stay on the device).  Same frame as ComputeWaves, bit for bit, and as a model without the twin."""
    import watersurfacerendering_amd as W
    n = 64
    xi = np.random.default_rng(5).standard_normal((n, n, 2)).astype(F)
    ws, plain = W.WSTessendorf(n, 1000.0, velocity=True), W.WSTessendorf(n, 1000.0)
    for m in (ws, plain):
        m.SetWindSpeed(20.0); m.SetLambda(-1.5)
        m.Prepare(seed=42, xi=xi)
    amp = ws.ComputeWaves(3.7)
    d, q, lo, hi = ws.GetDisplacements().copy(), ws.GetNormals().copy(), ws.GetMinHeight(), ws.GetMaxHeight()
    xz = np.random.default_rng(6).uniform(-500, 500, (65, 2)).astype(F)
    pos, vel = ws.QueryVelocity(xz)
    assert ws.ComputeWavesAsync(1.0) == ws.ComputeWaves(1.0)             # (another frame in between, through both paths)
    d1 = ws.GetDisplacements().copy()
    assert ws.ComputeWavesAsync(3.7) == amp
    assert np.array_equal(bits(ws.GetDisplacements()), bits(d1))         # still the previous frame's until Wait()
    ws.Wait()
    assert ws.GetDisplacements().shape == (n, n, 4) and ws.GetNormals().shape == (n, n, 4)
    assert np.array_equal(bits(ws.GetDisplacements()), bits(d)) and np.array_equal(bits(ws.GetNormals()), bits(q))
    assert (ws.GetMinHeight(), ws.GetMaxHeight()) == (lo, hi)
    pos2, vel2 = ws.QueryVelocity(xz)
    assert np.array_equal(bits(pos2), bits(pos)) and np.array_equal(bits(vel2), bits(vel))
    assert plain.ComputeWavesAsync(3.7) == amp
    plain.Wait()
    assert np.array_equal(bits(plain.GetDisplacements()), bits(d)) and np.array_equal(bits(plain.GetNormals()), bits(q))
    one = np.zeros((1, n, n, 4), F)
    with pytest.raises(ValueError):                                       # two tiles into arrays of one: refused before the library sees them
        ws._b.read_maps_async(one, one.copy())
