"""tests/half_intermediates.py, the float64 restatement of a frame with half2 intermediates, checked without a device: that it is the
oracle's frame when nothing is rounded, that it is the reduced path when something is, that its scale rule is ocean_prepare's, and that
the criterion tests/test_half_intermediates_gpu.py holds the kernels to tells a right rounding from a wrong one.

Measured (default Phillips sea, seed 0x5EED1600, t = 0 and 4.5, N = 16, 64, 256, both modes; every test prints its own):
    unquantised against numpy_compute_waves   4e-16 ... 1e-15 of a channel's maximum (1e-12 asserted)
    quantised against it                      5.7e-5 ... 3.3e-4 per channel (between the suite's TOL = 1e-5 and Z16_TOL = 1e-3)
    rounded toward zero / to nearest          rms ratio 1.40 ... 3.00 per channel (> 1 asserted)
    a z pass perturbed by 2e-7 of a column    rms ratio 0.01 ... 0.13, max ratio <= 0.58 (< 0.25 and <= 1 asserted)
    the aligned frame                         largest stored half 10363 (64^2), 14486 (512^2); 8567 at 64^2 in the Jacobian mode
"""
import numpy as np
import pytest

import half_intermediates as HI

TOL, Z16_TOL = 1e-5, 1e-3               # tests/test_parity_gpu.py
SEED = 0x5EED1600
SIZES = [16, 64, 256]
TIMES = (0.0, 4.5)
MODES = [False, True]


def mode_name(jac):
    return "jacobian" if jac else "full7"


_PREPS = {}


def prep_of(n):
    from oracle import oracle as O
    if n not in _PREPS:
        _PREPS[n] = O.numpy_prepare(n, O.gauss_xi_numpy(SEED, n))
    return _PREPS[n]


chan_err = HI.errors


@pytest.mark.parametrize("jac", MODES, ids=mode_name)
@pytest.mark.parametrize("n", SIZES)
def test_without_rounding_it_is_the_oracles_frame(n, jac):
    from oracle import oracle as O
    for t in TIMES:
        a, d, q, mn, mx = HI.frame(prep_of(n), t, -1.0, jac, quantise=False)
        ao, do, qo, mno, mxo = O.numpy_compute_waves(prep_of(n), t, lam=-1.0, jacobian=jac)
        err = chan_err(HI.channels(d, q), HI.channels(do, qo))
        print("n", n, mode_name(jac), "t", t, "worst channel", max(err), "A", abs(a - ao) / ao)
        assert max(err) <= 1e-12 and abs(a - ao) <= 1e-12 * ao and abs(mn - mno) <= 1e-12 * ao and abs(mx - mxo) <= 1e-12 * ao
        if jac:
            assert float(np.abs(do[..., 3] - 1.0).max()) > 1e-3             # the Jacobian slot is compared, and is not the constant
        pair = HI.frame_pair(prep_of(n), t, -1.0, jac)                      # (the large tiles' shortcut gives the same two frames)
        for got, want in ((pair[1], (a, d, q, mn, mx)), (pair[0], HI.frame(prep_of(n), t, -1.0, jac))):
            assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3:] == want[3:]


@pytest.mark.parametrize("jac", MODES, ids=mode_name)
@pytest.mark.parametrize("n", SIZES)
def test_with_rounding_it_is_the_reduced_path_inside_its_stated_accuracy(n, jac):
    from oracle import oracle as O
    for t in TIMES:
        info = {}
        a, d, q, _, _ = HI.frame(prep_of(n), t, -1.0, jac, info=info)
        ao, do, qo, _, _ = O.numpy_compute_waves(prep_of(n), t, lam=-1.0, jacobian=jac)
        err = chan_err(HI.channels(d, q), HI.channels(do, qo))
        live = [e for c, e in enumerate(err) if jac or c != 3]              # FULL7's w is the constant 1 in both
        print("n", n, mode_name(jac), "t", t, "channels", min(live), "...", max(live), "A", abs(a - ao) / ao, "largest stored", info["max_scaled"])
        assert TOL < min(live) and max(live) < Z16_TOL and abs(a - ao) < Z16_TOL * ao
        assert 0.0 < info["max_scaled"] <= 32768.0                          # the bound holds: nothing comes near 65504


def test_scale_rule_on_hand_made_bounds():
    """scale = the largest power of two with 4 bound scale <= 32768."""
    for e in (-20, -3, 0, 5, 11):                                           # exact powers of two: 32768 / (4 * 2^e) = 2^(13 - e), taken as it is
        s = HI.bound_scales(2.0 ** e, 2.0 ** (e + 2))
        assert s["su"] == 2.0 ** (13 - e) and s["sk"] == 2.0 ** (11 - e) and s["g"] == 0.25, s
        assert s["distance"]["su"] == 0.0 and s["distance"]["sk"] == 0.0 and s["distance"]["g"] == 0.0
        assert 4.0 * (2.0 ** e) * s["su"] == 32768.0
        assert s["s3"] == 2.0 ** (12 - e) and s["distance"]["s3"] == 0.0  # b0 + g b1 = 2 b0
    below, above = float(np.nextafter(np.float32(1.0), np.float32(0.0))), float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    s = HI.bound_scales(below, below)                                       # a bound just below a power of two: the quotient just above one
    assert s["su"] == 8192.0 and 0.0 < s["distance"]["su"] < 1e-6 and s["g"] == 1.0
    s = HI.bound_scales(above, above)                                       # just above: the next smaller power
    assert s["su"] == 4096.0 and 0.0 < s["distance"]["su"] < 1e-6
    assert 4.0 * above * s["su"] <= 32768.0 < 4.0 * above * 2.0 * s["su"]
    s = HI.bound_scales(3.0, 0.75)
    assert s["su"] == 2048.0 and s["sk"] == 8192.0 and s["g"] == 4.0 and s["s3"] == 1024.0      # 32768 / 12, / 3, 3 / 0.75, 32768 / 24
    assert abs(s["distance"]["su"] - 1.0 / 3.0) < 1e-12                                         # 2730.67: as far from 2048 as from 4096
    for b in (0.0, float("inf"), float("nan")):                             # nothing to bound, or no bound: 1
        s = HI.bound_scales(b, b)
        assert (s["su"], s["sk"], s["g"], s["s3"]) == (1.0, 1.0, 1.0, 1.0), (b, s)
    s = HI.bound_scales(2.0, 0.0)                                           # a spectrum at k = 0 only would have no k-weighted part
    assert s["su"] == 4096.0 and s["sk"] == 1.0 and s["g"] == 1.0 and s["s3"] == 4096.0
    for x, want in ((1.0, 0.0), (1.5, 0.25), (1.999, 0.0005), (1.001, 0.001), (3e-5 * 4 / 3, None)):
        got = HI.pow2_distance(x)
        assert 0.0 <= got <= 1.0 / 3.0 + 1e-12 and (want is None or abs(got - want) < 1e-12), (x, got)


def test_bounds_are_the_column_sums():
    """A spectrum with one heavy column: the bounds are that column's sums (a column is a fixed kx: the second index)."""
    n = 16
    p = prep_of(n)
    h0 = np.zeros((n, n), np.complex64)
    h0[:, 5] = 0.5 - 0.5j
    h0[3, :] += 0.25
    sc = HI.scales(h0, p["kx"], p["kz"])
    mag = np.abs(h0.astype(np.complex128))
    k = np.hypot(p["kx"].astype(np.float64), p["kz"].astype(np.float64))
    assert sc["b0"] == pytest.approx(float(mag[:, 5].sum()), rel=1e-12) and sc["b0"] > float(mag[3, :].sum())
    assert sc["b1"] == pytest.approx(max(float((mag * k)[:, j].sum()) for j in range(n)), rel=1e-12)
    assert HI.scales(np.zeros((n, n), np.complex64), p["kx"], p["kz"])["su"] == 1.0


def _gpu_inputs():
    import test_half_intermediates_gpu as G
    seen, out = set(), []
    for name, tl, h16 in G.all_inputs():
        key = repr((tl, h16))
        if key not in seen:                                                 # (the batches' tile 0 is the lone tile's spectrum)
            seen.add(key)
            out.append(pytest.param(tl, h16, id=name.replace(" ", "-")))
    return out


@pytest.mark.parametrize("tl,h16", _gpu_inputs())
def test_every_input_of_the_gpu_module_is_far_from_a_power_of_two(tl, h16):
    """The kernel sums its bounds in fp32 in an order of its own; the restated scale is the device's as long as the quotient it is
    taken from is not within rounding of a power of two.  Every spectrum tests/test_half_intermediates_gpu.py prepares keeps 1e-3."""
    import test_half_intermediates_gpu as G
    prep = G.numpy_prep(tl, G.draws(tl["n"], tl["kind"], tl["seed"]), h16=h16)
    sc = HI.scales(prep["h0"], prep["kx"], prep["kz"])
    print({k: round(v, 5) for k, v in sc["distance"].items()}, "su", sc["su"], "sk", sc["sk"], "g", sc["g"], "s3", sc["s3"])
    assert min(sc["distance"].values()) > G.DISTANCE, sc
    if h16:
        sc32 = HI.scales(prep["h0_fp32"], prep["kx"], prep["kz"])
        assert all(sc32[k] == sc[k] for k in ("su", "sk", "g", "s3")) and min(sc32["distance"].values()) > G.DISTANCE, sc32


def test_the_per_tile_case_has_scales_to_tell_apart():
    import test_half_intermediates_gpu as G
    sc = [HI.scales(p["h0"], p["kx"], p["kz"]) for p in (G.numpy_prep(tl, G.draws(64, tl["kind"], tl["seed"])) for tl in G.per_tile_tiles())]
    assert len({s["su"] for s in sc}) > 1 and len({s["sk"] for s in sc}) > 1 and len({s["s3"] for s in sc}) > 1, sc


@pytest.mark.parametrize("jac", MODES, ids=mode_name)
@pytest.mark.parametrize("n", SIZES)
def test_the_criterion_tells_rounding_toward_zero_from_rounding_to_nearest(n, jac):
    """The teeth: a frame whose stored halves were rounded toward zero lies further from the restatement, in every channel's rms, than
    the restatement lies from the oracle; one whose z pass was off by fp32 noise (2e-7 of a column's rms, the upper end of what an fp32
    transform does) lies four times nearer at least."""
    from oracle import oracle as O
    for t in TIMES:
        p = prep_of(n)
        rne = HI.frame(p, t, -1.0, jac)
        oracle = O.numpy_compute_waves(p, t, lam=-1.0, jacobian=jac)
        ref, orc = HI.channels(rne[1], rne[2]), HI.channels(oracle[1], oracle[2])
        rz = HI.frame(p, t, -1.0, jac, rounding="rz")
        noisy = HI.frame(p, t, -1.0, jac, noise=2e-7, seed=n)
        r_rz = [r for r, _ in HI.ratios(HI.channels(rz[1], rz[2]), ref, orc) if r is not None]
        r_noise = [r for r, _ in HI.ratios(HI.channels(noisy[1], noisy[2]), ref, orc) if r is not None]
        m_noise = [m for _, m in HI.ratios(HI.channels(noisy[1], noisy[2]), ref, orc) if m is not None]
        print("n", n, mode_name(jac), "t", t, "toward zero", min(r_rz), "...", max(r_rz), "| noise: rms", max(r_noise), "max", max(m_noise),
              "A", abs(noisy[0] - rne[0]) / rne[0])
        assert len(r_rz) == (8 if jac else 7)
        assert min(r_rz) > 1.0, r_rz
        assert max(r_noise) < 0.25, r_noise
        assert max(m_noise) <= 1.0 and abs(noisy[0] - rne[0]) <= 1e-5 * rne[0]


def test_rounding_toward_zero_is_toward_zero():
    x = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10 - 2.0 ** -20, -1.0 - 2.0 ** -11 - 2.0 ** -20, 65519.0, -70000.0, 2.0 ** -25, 3e-8, 0.0])
    assert np.array_equal(HI.to_half(x, "rz"), [1.0, 1.0, 1.0, -1.0, 65504.0, -65504.0, 0.0, 0.0, 0.0])
    assert np.array_equal(HI.to_half(x), [1.0, 1.0, 1.0 + 2.0 ** -10, -1.0 - 2.0 ** -10, 65504.0, -np.inf, 0.0, 2.0 ** -24, 0.0])      # ties to even; subnormals kept
    import half_maps as H
    t = H.boundary_table().astype(np.float64)
    t = t[np.isfinite(t)]
    assert np.array_equal(HI.to_half(t).astype(np.float16).view(np.uint16), H.rne_bits(t.astype(np.float32)))     # the integer-only conversion agrees


@pytest.mark.parametrize("jac", MODES, ids=mode_name)
@pytest.mark.parametrize("n", [64, 512])
def test_the_aligned_frame_stores_halves_of_4096_and_more(n, jac):
    """Draws (1, 0) at t = 0: every h0 is real and non-negative, so the height's row 0 of a column is that column's sum plus its
    mirror's, half of what the bound allows for.  The largest scaled magnitude is then at least 4096 (of 65504): a scale 8 times too
    large overflows on this frame, and the restatement says so."""
    import test_half_intermediates_gpu as G
    tl = G.tile(n, kind="aligned")
    prep = G.numpy_prep(tl, G.draws(n, "aligned", 0))
    assert np.all(prep["h0"].imag == 0) and np.all(prep["h0"].real >= 0) and prep["h0"].real.max() > 0
    info = {}
    a, d, q, _, _ = HI.frame(prep, 0.0, -1.0, jac, info=info)
    print("n", n, mode_name(jac), "largest stored", info["max_scaled"], info["scales"])
    assert 4096.0 <= info["max_scaled"] <= 32768.0 and np.all(np.isfinite(d)) and np.all(np.isfinite(q))
    assert 8.0 * info["max_scaled"] > 65520.0
    if not jac:                                                             # the height's row 0 of the heaviest column, as stated
        sc = info["scales"]
        col = np.abs(prep["h0"]).astype(np.float64).sum(axis=0)
        j = int(np.argmax(col))
        row0 = (col[j] + col[(n - j) % n]) * sc["su"]                      # S+ = h0(idx) + h0(-idx), summed down the column
        assert 4096.0 <= row0 <= info["max_scaled"] * (1 + 1e-6) and 8.0 * row0 > 65520.0, (row0, info)
