"""The fp16 copy of the spectrum (ocean_set_spectrum_precision(16): k_h0_absmax, k_h0_to_half, the H16 branch of zpass_load_pair) held to the
fp32 path's own bound.

The z pass reads float(half(h0 * 2^(14 - e))) * 2^(e - 14), e from frexpf of the tile's largest |component|, and behind that load the
frame IS the fp32 path.  So the float64 oracle fed that quantised spectrum -- tests/half_maps.quantise_h0 of the device's own h0, written
into the C oracle's h0 / h0_conj, which its compute path reads -- must be met to the fp32 bounds of tests/test_parity_gpu.py: every
channel's max|err| <= 1e-5 max|channel|; A, min and max within 1e-6 of A.  (tests/test_variants_gpu.py holds the same frames to 1e-3
against the oracle of the unquantised spectrum.)  At 1e-5 a wrong rounding mode, a maximum that misses part of a tile, a scale or an
inverse scale taken from another tile all show; that the bound tells the two spectra apart is asserted too: against the oracle of the
UNquantised spectrum every frame here must exceed 1e-5.

Measured on an MI355X, worst channel against the quantised oracle / against the unquantised one (every case prints its own):
    64^2   full7 6.0e-7 / 2.9e-4, jacobian 3.9e-7 / 2.9e-4        512^2  full7 and jacobian 7.5e-7 / 2.5e-4
    1024^2 one-column, single-transform (2 tiles) and two-column (16 tiles, depth 2) forms: 6.2e-7 / 3.1e-4, the same bits in all three
    batch with per-tile scales: 6.0e-7 / 2.9e-4 and 3.7e-7 / 2.2e-4; the zero tile is the flat sea exactly
    maximum at the first, the last and a late element: 4.6e-7 ... 1.1e-6 at 64^2, 3.9e-7 ... 8.0e-7 at 1024^2
so the worst case of the file is 1.1e-6 against a bound of 1e-5, and the unquantised oracle is 20 to 30 bounds away.
"""
import time

import numpy as np
import pytest

import half_maps as H

pytestmark = pytest.mark.gpu

TOL, TOL_AMP = 1e-5, 1e-6
SEED = 0x5EED0000
T_FRAME = 1.7
FLT_MIN = np.float32(np.finfo(np.float32).tiny)


def chan_err(a, b):
    out = []
    for c in range(4):
        den = max(float(np.abs(b[..., c]).max()), 1e-30)
        out.append(float(np.abs(a[..., c].astype(np.float64) - b[..., c]).max()) / den)
    return out


def feed(o, h0, omega=None):
    """Replace a prepared C oracle's spectrum: h0 and the per-bin conjugate its compute path adds (for a Phillips sea h0_conj is
    conj(h0) of the same bin: both directions have the same P), and the device's omega."""
    assert np.array_equal(o.h0_conj[..., 0], o.h0[..., 0]) and np.array_equal(o.h0_conj[..., 1], -o.h0[..., 1])
    o.h0[...] = h0
    o.h0_conj[..., 0] = h0[..., 0]
    o.h0_conj[..., 1] = -h0[..., 1]
    if omega is not None:
        assert np.array_equal(o.omega, omega)                   # (test_device_init_matches_oracle: bit-equal)
        o.omega[...] = omega


def oracle_frame(n, xi, h0, omega, jac, t=T_FRAME, **params):
    """(A, disp, nrm, min, max) of the float64-FFT oracle on the spectrum h0 (xi only prepares k, omega and the buffers)."""
    from oracle import oracle as O
    o = O.Oracle(n, **params)
    o.prepare(xi=xi)
    feed(o, h0, omega)
    a, d, q = o.compute_waves(t, mode=O.MODE_JACOBIAN if jac else O.MODE_FULL7, fft=O.FFT_F64)
    return a, d, q, o.min_height, o.max_height


def meets(d, q, h, ref, jac, what):
    """The fp32 path's bounds; returns the worst channel error."""
    ao, do, no, mn, mx = ref
    assert np.all(np.isfinite(d)) and np.all(np.isfinite(q)), what
    assert abs(h[0] - ao) <= TOL_AMP * abs(ao), (what, h[0], ao)
    assert abs(h[1] - mn) <= TOL_AMP * abs(ao) and abs(h[2] - mx) <= TOL_AMP * abs(ao), (what, h, mn, mx)
    ed, en = chan_err(d, do), chan_err(q, no)
    if max(ed + en) > TOL:
        import spectra
        raise AssertionError((what, "displacement", ed, "normal", en, "worst bins (channel, (row, column), share)",
                              spectra.worst_bins(d, do), spectra.worst_bins(q, no)))
    if jac:
        assert float(np.abs(do[..., 3] - 1.0).max()) > 1e-3, what              # displacement.w is compared, and is not the constant
    else:
        assert np.all(d[..., 3] == 1.0), what
    return max(ed + en)


def fp16_frame(n, tiles, depth, jac, xi=None, seed=SEED, tile_params=None, t=T_FRAME):
    """One frame at t with the fp16 spectrum: ([(disp, nrm, heights, xi, h0, omega) per tile], launch records)."""
    import watersurfacerendering_amd as W
    from watersurfacerendering_amd import _abi as A
    b = W.OceanBatch(n, tiles, 0)
    for i, p in enumerate(tile_params or ()):
        b.set_params(tile=i, **p)
    b.set_spectrum_precision(16)
    b.set_mode(A.OCEAN_MODE_JACOBIAN if jac else A.OCEAN_MODE_FULL7)
    b.set_pipeline_depth(depth)
    b.prepare(seed, xi)
    for j in range(depth - 1):                 # (as tests/test_variants_gpu.run_frame: the checked frame runs beside frames in flight)
        b.compute_waves_async(0.3 * j)
    if depth > 1:
        b.compute_waves_async(t)
        b.synchronize()
    else:
        b.compute_waves(t)
    launches = b.last_launch()
    count = tiles if tile_params else 1
    d, q = b.read_maps(0, count)
    out = []
    for i in range(count):
        h0, om = b.read_spectrum(i)
        out.append((d[i], q[i], b.heights(i), b.read_xi(i), h0, om))
    b.close()
    return out, launches


def z_form(launches):
    """Which z pass ran, from ocean_last_launch; asserts that it read the fp16 copy."""
    from watersurfacerendering_amd import _abi as A
    z = launches[0]
    assert z["flags"] & A.OCEAN_LAUNCH_FP16_SPECTRUM, z
    if z["flags"] & A.OCEAN_LAUNCH_SINGLE_TRANSFORM:
        assert z["per_workgroup"] == 1
        return "single-transform"
    return {1: "one-column", 2: "two-column"}[z["per_workgroup"]]


def both_errors(d, q, h, xi, h0, om, jac, what, **params):
    """Meets the oracle of the quantised spectrum, misses the oracle of the unquantised one; prints and returns both worst errors."""
    n = h0.shape[0]
    hq = H.quantise_h0(h0)
    assert not np.array_equal(hq, h0)
    err_q = meets(d, q, h, oracle_frame(n, xi, hq, om, jac, **params), jac, what)
    _, do, no, _, _ = oracle_frame(n, xi, h0, om, jac, **params)
    err_u = max(chan_err(d, do) + chan_err(q, no))
    print(f"fp16 spectrum {what}: worst channel {err_q:.3e} against the quantised oracle, {err_u:.3e} against the unquantised one")
    assert err_u > TOL, (what, err_u)
    return err_q, err_u


# (n, tiles, depth, jacobian, the z-pass form that must run); "stream" of tests/test_variants_gpu.policies(1024) is 16 tiles at depth 2
CASES = [(64, 1, 1, False, "one-column"), (64, 1, 1, True, "one-column"),
         (512, 1, 1, False, "one-column"), (512, 1, 1, True, "one-column"),      # 512^2: exactly one element per thread of k_h0_absmax
         (1024, 1, 1, False, "one-column"),                                        # four trips of k_h0_absmax / k_h0_to_half
         (1024, 2, 1, False, "single-transform"),
         (1024, 16, 2, False, "two-column")]


@pytest.mark.parametrize("n,tiles,depth,jac,form", CASES)
def test_fp16_spectrum_frame_meets_the_fp32_bound_against_the_quantised_oracle(n, tiles, depth, jac, form):
    import test_variants_gpu as V
    if (n, tiles, depth) == (1024, 16, 2):
        assert ("stream", tiles, depth) in V.policies(n)
    t0 = time.perf_counter()
    (tile0,), launches = fp16_frame(n, tiles, depth, jac)
    assert z_form(launches) == form and launches[0]["tile_size"] == n and launches[0]["grid_y"] == tiles
    both_errors(*tile0, jac, (n, tiles, depth, "jacobian" if jac else "full7", form))
    print(f"wall time {time.perf_counter() - t0:.2f} s")


def test_fp16_spectrum_batch_with_per_tile_scales():
    """Three 64^2 tiles whose spectra differ by 10^4 in power, the third zero: every tile is scaled by its own maximum and read back with
    its own inverse scale; the zero tile (maximum 0: e = 0) is the flat sea exactly."""
    n = 64
    consts = (3e-7, 3e-3, 0.0)
    tiles, launches = fp16_frame(n, 3, 1, False, tile_params=[dict(phillips_const=a) for a in consts])
    assert z_form(launches) == "one-column" and launches[0]["grid_y"] == 3
    exps = [H.h0_exponent(t[4]) for t in tiles]
    assert exps[1] - exps[0] >= 4 and exps[2] == 0, exps                       # sqrt(10^4) = 2^6.6 (and other draws): the scales really differ
    for i in (0, 1):
        both_errors(*tiles[i], False, (n, "tile", i, "phillips_const", consts[i]), phillips_a=consts[i])
    d, q, h, _, h0, _ = tiles[2]
    assert not h0.any()
    assert h[0] == float(FLT_MIN), h                                           # A = FLT_MIN: the running maximum starts there
    assert not d[..., :3].any() and np.all(d[..., 3] == 1.0) and not q.any()   # height 0, w = 1, everything else 0


def max_elements(n):
    """Transposed elements (the device stores wave (m, q) at q * n + m) where the tile's maximum is put: the first, the last, and one
    that k_h0_absmax's fixed grid of 1024 x 256 threads reaches late -- at 1024^2 thread 17 of workgroup 1023 on its fourth and last
    trip; at 64^2 (4096 elements: workgroups 16 .. 1023 have none) an element of another workgroup and wave than the first two."""
    late = 3 * 1024 * 256 + 1023 * 256 + 17 if n == 1024 else 9 * 256 + 64 + 41
    assert late < n * n
    return (0, n * n - 1, late)


@pytest.mark.parametrize("n", [64, 1024])
def test_fp16_spectrum_finds_its_maximum_wherever_it_sits(n):
    """Injected draws of 1e-3 everywhere and one of 1e3: that bin is the tile's maximum by so much that a maximum taken without it
    scales it beyond 65504 -- inf in the copy, NaN in the maps.  With it, the frame meets the bounds."""
    t0 = time.perf_counter()
    for el in max_elements(n):
        m, q = el % n, el // n
        xi = np.full((1, n, n, 2), 1e-3, np.float32)
        xi[0, m, q] = (-1e3, 1e-3)
        ((d, nr, h, xi_dev, h0, om),), launches = fp16_frame(n, 1, 1, False, xi=xi)
        assert np.array_equal(xi_dev, xi[0]) and z_form(launches) == "one-column"
        mag = np.abs(h0).max(axis=-1)
        assert np.unravel_index(int(np.argmax(mag)), mag.shape) == (m, q), (n, el)
        rest = mag.copy(); rest[m, q] = 0.0
        assert float(mag[m, q]) * 2.0 ** (14 - H.h0_exponent(rest)) >= 65520.0, (n, el)     # missed, it would overflow the half
        what = (n, "maximum at transposed element", el, "wave", (m, q))
        err_q = meets(d, nr, h, oracle_frame(n, xi[0], H.quantise_h0(h0), om, False), False, what)
        print(f"fp16 spectrum {what}: worst channel {err_q:.3e} against the quantised oracle")
    print(f"wall time {time.perf_counter() - t0:.2f} s")
