"""Empirical spectra on the MI355X (include/ocean_consumers.h: ocean_set_spectrum, ocean_get_spectrum, ocean_spectrum_moments): the
prepared spectrum against its float64 restatement (tests/empirical_spectra.py) to 2 ulp, the default sea and the Phillips bits left
alone, bands that partition a cascade set, frames of the new sea against the float64 oracle at the suite's bounds, the moments, twins
and the fp16 spectrum copy.

The 2 ulp: sp = (float)(scale * sqrt(P)) is a double result rounded once on both sides; device and numpy libm differ by ~1e-15
relatively, so sp differs by at most one ulp, and the one fp32 product behind it adds at most one more (2^-148 absolutely below
FLT_MIN, where an ulp is 2^-149)."""
import numpy as np
import pytest

import empirical_spectra as E
import velocity as V

pytestmark = pytest.mark.gpu
F = np.float32
TOL, TOL_AMP = 1e-5, 1e-6               # the suite's parity bounds (tests/test_parity_gpu.py)
FP16_TOL = 1e-3                         # ... and the one it states for the fp16 spectrum (test_fp16_spectrum_within_stated_tolerance)
WIND, U = (1.0, 0.4142135), 10.0
LENGTHS = {16: 150.0, 64: 500.0, 256: 500.0}        # the JONSWAP peak (k_p ~ 0.1 rad/m at U = 10, F = 100 km) lies inside every lattice


def sea(n, **kw):
    return dict(dict(length=LENGTHS[n], wind=WIND, wind_speed=U), **kw)


def gpu_params(s):
    return dict(tile_length=s["length"], wind_dir_x=s["wind"][0], wind_dir_y=s["wind"][1], wind_speed=s["wind_speed"])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pairs(h0c):
    return np.stack([h0c.real, h0c.imag], axis=-1).astype(F)


def band_edges(n):
    """Two wavenumbers strictly inside the lattice of the n-tile, not on a lattice circle: the bands they bound cut it."""
    dk = 2.0 * np.pi / LENGTHS[n]
    return 0.115 * n * dk, 0.31 * n * dk


def specs_of(n):
    k1, k2 = band_edges(n)
    return [
        E.spectrum(kind=E.PM),
        E.spectrum(kind=E.PM, spreading=E.HASSELMANN),
        E.spectrum(kind=E.JONSWAP, swell=0.5, spread_s=3.0),
        E.spectrum(kind=E.JONSWAP, spreading=E.HASSELMANN),
        E.spectrum(kind=E.TMA, depth=12.0, scale=0.5),
        E.spectrum(kind=E.TMA, spreading=E.HASSELMANN, alpha=0.01, peak_omega=0.9, fetch=30e3, gamma=2.0),
        E.spectrum(kind=E.JONSWAP, spreading=E.HASSELMANN, k_min=k1, k_max=k2),
        E.spectrum(kind=E.JONSWAP, spreading=E.HASSELMANN, k_max=k1),
    ]


@pytest.mark.parametrize("dispersion", [(0, 0.0), (1, 15.0)], ids=["deep", "finite_depth"])
@pytest.mark.parametrize("injected", [False, True], ids=["generated", "injected"])
@pytest.mark.parametrize("n", [16, 64])
def test_prepared_spectrum_is_the_restatement_to_two_ulp(n, injected, dispersion):
    import watersurfacerendering_amd as W
    from oracle import oracle as O
    specs = specs_of(n)
    s = sea(n)
    seed = 0x5EA5
    xi_in = np.stack([O.gauss_xi_numpy(77 + i, n) for i in range(len(specs))]) if injected else None
    plain = W.OceanBatch(n, len(specs), 0)          # the default sea of the same parameters: whose omega and draws must not move
    b = W.OceanBatch(n, len(specs), 0)
    for c in (plain, b):
        c.set_params(**gpu_params(s))
        c.set_dispersion(*dispersion)
    for i, sp in enumerate(specs):
        b.set_spectrum(i, **sp)
    plain.prepare(seed, xi_in)
    b.prepare(seed, xi_in)
    worst = 0.0
    for i, sp in enumerate(specs):
        h0, om = b.read_spectrum(i)
        xi = b.read_xi(i)
        _, om0 = plain.read_spectrum(i)
        assert np.array_equal(bits(om), bits(om0)) and np.array_equal(bits(xi), bits(plain.read_xi(i))), i
        if injected:
            assert np.array_equal(bits(xi), bits(xi_in[i])), i
        prep = O.numpy_prepare(n, xi, dispersion=dispersion, **s)
        want = pairs(E.restate_h0(prep, xi, sp, dispersion_kind=dispersion, **s))
        ulp = E.ulp_distance(h0, want)
        worst = max(worst, float(ulp.max()))
        print("n", n, "injected", injected, "dispersion", dispersion, "tile", i, "max ulp", float(ulp.max()), "max|h0|", float(np.abs(want).max()))
        assert np.all(np.isfinite(h0)) and float(np.abs(want).max()) > (1e-4 if i < 6 else 0.0), i       # (a band may hold little of the energy)
        assert float(ulp.max()) <= 2.0, (i, float(ulp.max()))
        keep = E.in_band(prep, sp)
        keep[n // 2, n // 2] = False
        assert np.all(bits(h0)[~keep] == 0), i                                  # DC and out of band: exactly +0
        if i >= 6:
            assert 0 < int(keep.sum()) < n * n - 1 and np.any(h0[keep] != 0), i     # the band cuts the lattice
        g = b.spectrum(i)
        a, wp, _ = E.resolve(sp, U)
        assert g.kind == sp["kind"] and g.alpha == F(a) and g.peak_omega == F(wp), i
    print("worst ulp", worst)
    plain.close(); b.close()


def test_default_tiles_and_phillips_bits_are_untouched():
    import watersurfacerendering_amd as W
    n, seed = 64, 0xD0
    s = sea(n, wind_speed=12.0)
    k1, k2 = band_edges(n)
    plain = W.OceanBatch(n, 3, 0)
    b = W.OceanBatch(n, 3, 0)
    for c in (plain, b):
        c.set_params(**gpu_params(s))
    b.set_spectrum(0, **E.spectrum())                                       # ocean_default_spectrum, set explicitly
    b.set_spectrum(1, **E.spectrum(kind=E.JONSWAP))
    b.set_spectrum(2, **E.spectrum(k_min=k1, k_max=k2))                     # Phillips in a band
    plain.prepare(seed); b.prepare(seed)
    for c in (plain, b):
        c.compute_waves(1.75)
    h0, om = b.read_spectrum(0)
    h0p, omp = plain.read_spectrum(0)
    assert np.array_equal(bits(h0), bits(h0p)) and np.array_equal(bits(om), bits(omp)) and np.abs(h0).max() > 0
    for got, ref in zip(b.read_maps(0, 1), plain.read_maps(0, 1)):
        assert np.array_equal(bits(got), bits(ref))
    assert not np.array_equal(bits(b.read_spectrum(1)[0]), bits(plain.read_spectrum(1)[0]))
    from oracle import oracle as O
    keep = E.in_band(O.numpy_prepare(n, b.read_xi(2), **s), E.spectrum(k_min=k1, k_max=k2))
    h2, om2 = b.read_spectrum(2)
    h2p, om2p = plain.read_spectrum(2)
    assert 0 < int(keep.sum()) < n * n and np.any(h2p[~keep] != 0)
    assert np.array_equal(bits(h2)[keep], bits(h2p)[keep]) and np.all(bits(h2)[~keep] == 0) and np.array_equal(bits(om2), bits(om2p))
    # host state: it survives another prepare and a change of tile size, and going back to the default gives the default bits back
    b.set_tile_size(32); b.set_tile_size(n)
    assert b.spectrum(1).kind == E.JONSWAP and b.spectrum(2).k_max == F(k2)
    b.prepare(seed)
    assert np.array_equal(bits(b.read_spectrum(2)[0]), bits(h2))
    b.set_spectrum(2, k_min=0.0, k_max=0.0)
    b.prepare(seed)
    assert np.array_equal(bits(b.read_spectrum(2)[0]), bits(h2p))
    plain.close(); b.close()


@pytest.mark.parametrize("n", [16, 64])
def test_bands_partition_a_cascade_set_bit_for_bit(n):
    import watersurfacerendering_amd as W
    from oracle import oracle as O
    s = sea(n)
    k1, _ = band_edges(n)
    xi = O.gauss_xi_numpy(5, n)
    b = W.OceanBatch(n, 3, 0)
    b.set_params(**gpu_params(s))
    b.set_spectrum(kind=E.JONSWAP, spreading=E.HASSELMANN)
    b.set_spectrum(0, k_max=k1)
    b.set_spectrum(1, k_min=k1)
    b.prepare(0, np.stack([xi] * 3))
    low, high, full = (b.read_spectrum(i)[0] for i in range(3))
    assert np.any(low != 0) and np.any(high != 0)
    assert not np.any((low != 0).any(-1) & (high != 0).any(-1))             # every bin lives in exactly one of the two
    assert np.array_equal(bits(low + high), bits(full))
    m = [b.spectrum_moments(i) for i in range(3)]
    assert np.allclose(m[0] + m[1], m[2], rtol=1e-12, atol=0.0)
    b.close()


@pytest.mark.parametrize("jacobian", [False, True], ids=["full7", "jacobian"])
@pytest.mark.parametrize("n", [64, 256])
def test_frames_of_a_jonswap_sea_meet_the_suites_bounds(n, jacobian):
    import watersurfacerendering_amd as W
    from oracle import oracle as O
    from watersurfacerendering_amd import _abi
    s = sea(n)
    sp = E.spectrum(kind=E.JONSWAP, spreading=E.HASSELMANN)
    xi = O.gauss_xi_numpy(0x5EED + n, n)
    b = W.OceanBatch(n, 1, 0)
    b.set_params(**gpu_params(s))
    b.set_spectrum(0, **sp)
    b.set_mode(_abi.OCEAN_MODE_JACOBIAN if jacobian else _abi.OCEAN_MODE_FULL7)
    b.prepare(0, xi[None])
    prep = O.numpy_prepare(n, xi, **s)
    prep["h0"] = E.restate_h0(prep, xi, sp, **s)
    h0_dev, om_dev = b.read_spectrum(0)
    assert np.array_equal(bits(om_dev), bits(prep["omega"]))
    prep_dev = dict(prep, h0=V.as_complex(h0_dev))
    for t in (0.0, 3.25):
        amp = float(b.compute_waves(t)[0])
        d, q = b.read_maps(0, 1)
        a, rd, rq, _, _ = O.numpy_compute_waves(prep, t, lam=-1.0, jacobian=jacobian)
        a_dev = O.numpy_compute_waves(prep_dev, t, lam=-1.0, jacobian=jacobian)[0]
        print("n", n, "jacobian", jacobian, "t", t, "A", amp, "oracle", a, "rel", abs(amp - a_dev) / a_dev, "Hs", 4.0 * np.sqrt(b.spectrum_moments(0)[0]))
        for name, got, ref in (("disp", d[0], rd), ("nrm", q[0], rq)):
            for c in range(4):
                m = float(np.abs(ref[..., c]).max())
                err = float(np.abs(got[..., c].astype(np.float64) - ref[..., c]).max())
                print("  ", name, c, "max|ref|", m, "err/max", err / m)
                assert m > 0.0 and err <= TOL * m, (n, jacobian, t, name, c, err / m)
        assert abs(amp - a_dev) <= TOL_AMP * a_dev, (amp, a_dev)
        assert 0.05 < a < 5.0                                               # metres: a 10 m/s sea, not 3e-7 of something
    b.close()


@pytest.mark.parametrize("n", [16, 64, 256])
def test_moments_are_the_float64_sums_and_repeat_bit_for_bit(n):
    import watersurfacerendering_amd as W
    from oracle import oracle as O
    from watersurfacerendering_amd import _abi
    s = sea(n)
    b = W.OceanBatch(n, 2, 0)
    with pytest.raises(W.OceanError) as e:
        b.spectrum_moments(0)
    assert e.value.code == _abi.OCEAN_E_NOT_READY
    b.set_params(**gpu_params(s))
    b.set_spectrum(1, kind=E.JONSWAP, spreading=E.HASSELMANN)
    b.prepare(31)
    for i in range(2):
        h0, _ = b.read_spectrum(i)
        prep = O.numpy_prepare(n, b.read_xi(i), **s)
        k = E.wavenumber_f32(prep).astype(np.float64)
        p = h0[..., 0].astype(np.float64) ** 2 + h0[..., 1].astype(np.float64) ** 2
        want = np.array([p.sum(), (k * p).sum(), (k * k * p).sum()])
        got = b.spectrum_moments(i)
        print("n", n, "tile", i, "moments", got, "rel", np.abs(got - want) / want)
        assert np.all(want > 0) and np.all(np.abs(got - want) <= 1e-10 * want), (i, got, want)
        assert np.array_equal(got.view(np.uint64), b.spectrum_moments(i).view(np.uint64))
    with pytest.raises(W.OceanError):
        b.spectrum_moments(2)
    b.close()


def test_significant_wave_height_is_four_root_m0():
    """Draws (1, 1) make |h0|^2 = P exactly (up to the rounding of sp), so sum |h0|^2 is the lattice sum of the CPU energy test: at
    256^2, L = 500, U = 10 it is within 2 % of m0 = integral of S d omega, Hs within 1 %."""
    import watersurfacerendering_amd as W
    n = 256
    s = sea(n)
    deep = [E.spectrum(kind=E.PM), E.spectrum(kind=E.PM, spreading=E.HASSELMANN), E.spectrum(kind=E.JONSWAP, spreading=E.HASSELMANN, fetch=100e3),
            E.spectrum(kind=E.JONSWAP, swell=0.5)]
    b = W.OceanBatch(n, len(deep), 0)
    b.set_params(**gpu_params(s))
    ones = np.ones((len(deep), n, n, 2), F)

    def check(i, sp):
        m0 = E.variance_integral(sp, U)
        got = float(b.spectrum_moments(i)[0])
        hs, want = 4.0 * np.sqrt(got), 4.0 * np.sqrt(m0)
        print("kind", sp["kind"], "spreading", sp["spreading"], "m0", got, "integral", m0, "Hs", hs, "expected", want)
        assert abs(got - m0) <= 0.02 * m0 and abs(hs - want) <= 0.01 * want

    for i, sp in enumerate(deep):
        b.set_spectrum(i, **sp)
    b.prepare(0, ones)
    for i, sp in enumerate(deep):
        check(i, sp)
    tma = E.spectrum(kind=E.TMA, depth=20.0)
    b.set_spectrum(0, **tma)
    b.set_dispersion(1, 20.0)
    b.prepare(0, ones)
    check(0, tma)
    b.close()


def test_a_twin_is_the_derivative_of_the_new_spectrum():
    import watersurfacerendering_amd as W
    from watersurfacerendering_amd import _abi
    n = 64
    s = sea(n)
    b = W.OceanBatch(n, 2, 0)
    b.set_params(**gpu_params(s))
    b.set_velocity_twin(1, 0)
    b.set_spectrum(kind=E.JONSWAP, spreading=E.HASSELMANN)                  # ALL_TILES skips the twin
    with pytest.raises(W.OceanError) as e:
        b.set_spectrum(1, kind=E.PM)
    assert e.value.code == _abi.OCEAN_E_INVALID
    assert b.spectrum(1).kind == E.JONSWAP                                  # the source's
    b.prepare(9)
    h0, om = b.read_spectrum(0)
    th0, tom = b.read_spectrum(1)
    assert np.abs(h0).max() > 1e-3 and np.array_equal(bits(tom), bits(om))
    assert np.array_equal(bits(th0), bits(V.derive_spectrum(h0, om)))
    b.compute_waves(2.0)
    xz = np.array([[0.0, 0.0], [13.5, -40.25], [-220.0, 75.0]], F)
    pos, vel = b.query_velocity(xz, first_tile=0, grid_size=n, vertex_distance=s["length"] / n)
    assert np.all(np.isfinite(pos)) and np.all(np.isfinite(vel)) and np.abs(vel[:, :3]).max() > 0
    b.close()


def test_fp16_spectrum_copy_of_an_empirical_tile():
    """ocean_set_spectrum_precision(16): the half2 copy is made from the shaped spectrum, and one frame keeps the bound the suite
    states for a Phillips sea in that variant (FP16_TOL of each channel's maximum; the Jacobian slot is not compared there)."""
    import watersurfacerendering_amd as W
    from oracle import oracle as O
    n, t = 64, 4.5
    s = sea(n)
    sp = E.spectrum(kind=E.JONSWAP, spreading=E.HASSELMANN)
    xi = O.gauss_xi_numpy(404, n)
    b = W.OceanBatch(n, 1, 0)
    b.set_params(**gpu_params(s))
    b.set_spectrum(0, **sp)
    b.set_spectrum_precision(16)
    b.prepare(0, xi[None])
    prep = O.numpy_prepare(n, xi, **s)
    prep["h0"] = E.restate_h0(prep, xi, sp, **s)
    a, rd, rq, _, _ = O.numpy_compute_waves(prep, t, lam=-1.0)
    amp = float(b.compute_waves(t)[0])
    d, q = b.read_maps(0, 1)
    assert abs(amp - a) <= FP16_TOL * a
    worst = 0.0
    for got, ref, chans in ((d[0], rd, 3), (q[0], rq, 4)):
        for c in range(chans):
            m = float(np.abs(ref[..., c]).max())
            worst = max(worst, float(np.abs(got[..., c].astype(np.float64) - ref[..., c]).max()) / m)
    print("fp16 spectrum, worst channel error / max", worst)
    assert worst <= FP16_TOL
    b.close()


def test_set_spectrum_refuses_what_the_header_lists():
    import watersurfacerendering_amd as W
    from watersurfacerendering_amd import _abi
    b = W.OceanBatch(16, 2, 0)
    bad = [dict(kind=4), dict(spreading=2), dict(fetch=0.0), dict(fetch=-1.0), dict(gamma=0.0), dict(spread_s=0.0), dict(spread_s=-2.0),
           dict(scale=0.0), dict(scale=-1.0), dict(kind=E.TMA, depth=0.0), dict(kind=E.TMA, depth=-3.0), dict(swell=-0.1), dict(swell=1.5),
           dict(alpha=-1e-3), dict(peak_omega=-1.0), dict(k_min=-0.1), dict(k_max=-0.1), dict(k_min=0.5, k_max=0.5), dict(k_min=0.5, k_max=0.25)]
    bad += [{f: v} for f in ("fetch", "gamma", "depth", "spread_s", "swell", "alpha", "peak_omega", "k_min", "k_max", "scale")
            for v in (float("nan"), float("inf"))]
    for fields in bad:
        with pytest.raises(W.OceanError) as e:
            b.set_spectrum(0, **fields)
        assert e.value.code == _abi.OCEAN_E_INVALID, fields
    with pytest.raises(W.OceanError) as e:
        b.set_spectrum(2, kind=E.PM)                                        # outside the batch
    assert e.value.code == _abi.OCEAN_E_INVALID
    with pytest.raises(W.OceanError):
        b.spectrum(2)
    assert b._L.ocean_set_spectrum(b._h, 0, None) == _abi.OCEAN_E_INVALID
    assert b._L.ocean_get_spectrum(b._h, 0, None) == _abi.OCEAN_E_INVALID
    assert b._L.ocean_spectrum_moments(b._h, 0, None) == _abi.OCEAN_E_INVALID
    assert b.spectrum(0).kind == E.PHILLIPS                                 # nothing of the refused calls stuck
    b.set_spectrum(0, kind=E.PM, depth=0.0)                                 # depth matters for TMA only
    b.set_spectrum(1, k_min=0.25)                                           # k_max == 0: no upper limit
    assert (b.spectrum(0).kind, b.spectrum(1).k_min) == (E.PM, 0.25)
    b.close()
