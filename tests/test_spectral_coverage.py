"""The inputs of tests/test_spectral_coverage_gpu.py, checked on the CPU (tests/spectra.py).

  * construction: the white spectrum puts |h0| = AMP on every bin but DC and the few capped ones (99.85 % of the bins at 4096^2, the
    Nyquist row and column at least 99.4 %), the edge spectrum exactly on its lines, the sparse one on its bins;
  * the closed form (no FFT) equals the C oracle's float64-FFT frame on the sparse spectrum in every mode, at t = 0, 7.25 and 3e5 --
    which pins the oracle at the edge bins, where Phillips inputs never looked;
  * sensitivity, a mutation argument run on the oracle: zeroing the Nyquist column or row, or the single bin (0, 1) or (1, 0), moves the
    new inputs' maps far above the GPU tests' 1e-5 -- on the Phillips inputs of the rest of the suite the same mutations stay below it
    (7e-9 for the whole Nyquist column at 4096^2 with the ALT parameters), so only the new tests can see such a kernel bug;
  * the oracle's own fp32 transforms stay within 1e-6 of the float64 frame on the white input: a flat spectrum needs no looser
    tolerance than a sea.
"""
import numpy as np
import pytest

import spectra as S

T = 7.25
TOL_CLOSED = 2e-7           # closed form vs the FFT_F64 frame: the fp32 rounding of the oracle's stored maps (measured <= 1.4e-7)
TOL_CLOSED_JAC = 4e-7       # its Jacobian channel: four fp32 products of rounded fields (measured <= 2.0e-7)


def oracle_frame(n, xi, mode, fft=None):
    from oracle import oracle as O
    o = S.make_oracle(n, xi)
    a, d, q = o.compute_waves(T, mode=mode, fft=O.FFT_F64 if fft is None else fft)
    return a, np.concatenate([d, q], axis=-1)


@pytest.mark.parametrize("n", [16, 64, 256, 1024, 2048, 4096])
def test_white_and_edge_spectra_reach_every_bin(n):
    from oracle import oracle as O
    xi = S.white_xi(n, 3)[0]
    o = S.make_oracle(n, xi)
    h = np.abs(o.h0.astype(np.float64) @ np.array([1.0, 1j]))
    u = S.unit(n)
    dc = (n // 2, n // 2)
    on = np.abs(h - S.AMP) <= 1e-3 * S.AMP
    off = h == 0
    assert np.all(on | off)                                              # every bin is either at the target amplitude or unexcited
    assert np.array_equal(off, u < S.AMP * S.CAP) and off[dc]            # ... and unexcited only where the cap says so (DC included)
    assert on.mean() >= {4096: 0.9985, 2048: 0.9996, 1024: 0.9999}.get(n, 1.0 - 1.0 / (n * n))
    assert on[0].mean() >= 0.994 and on[:, 0].mean() >= 0.994           # the Nyquist row and column
    for b in [(0, 1), (1, 0), (0, n - 1), (n - 1, 0), (n // 2, 0), (0, n // 2), (n - 1, n - 1), (0, 0)]:
        assert on[b], b
    e = S.edge_xi(n, 3)[0]
    mask = S.edge_mask(n)
    assert np.all(e[~mask] == 0) and np.array_equal(e[mask], xi[mask])
    for line in S.edge_lines(n):
        assert min(np.count_nonzero(on[line]), np.count_nonzero(on[:, line])) >= 0.99 * n - 1       # (line N/2 holds DC)
    sp = S.sparse_xi(n)[0]
    o = S.make_oracle(n, sp)
    excited = set(zip(*np.nonzero((o.h0 != 0).any(axis=-1))))
    assert excited == set(S.sparse_bins(n)) - {dc} and len(excited) >= (15 if n == 16 else 28)
    assert np.any(sp[dc] != 0) and np.all(o.h0[dc] == 0)
    mags = sorted(float(np.hypot(*o.h0[b])) for b in excited)
    assert mags[0] >= 0.29 * S.AMP and mags[-1] <= 1.01 * S.AMP
    assert O.MODE_FULL7 == 0 and O.MODE_JACOBIAN == 3


@pytest.mark.parametrize("n", [16, 32, 64, 128, 256, 512, 1024])
def test_closed_form_equals_the_oracle_on_the_sparse_spectrum(n):
    from oracle import oracle as O
    o = S.make_oracle(n, S.sparse_xi(n)[0])
    sp = S.spectrum_of(o)
    lam = S.PARAMS["lam"]
    for mode in range(4):
        for t in (0.0, 7.25, 3e5):
            a, d, q, mn, mx = S.closed_form(sp, t, lam, mode)
            ao, do, no = o.compute_waves(t, mode=mode, fft=O.FFT_F64)
            what = (n, S.MODES[mode], t)
            assert abs(ao - a) <= 1e-6 * a and abs(o.min_height - mn) <= 1e-6 * a and abs(o.max_height - mx) <= 1e-6 * a, what
            ed, en = S.chan_err(do, d), S.chan_err(no, q)
            assert max(ed[:3] + en) <= TOL_CLOSED, (what, ed, en, S.worst_bins(np.concatenate([do, no], -1), np.concatenate([d, q], -1)))
            assert ed[3] <= (TOL_CLOSED_JAC if mode == 3 else 0.0), (what, ed)
            if mode == 3:
                assert float(np.abs(d[..., 3] - 1.0).max()) > 1e-3, what       # a real Jacobian, not the constant 1


@pytest.mark.parametrize("n", [1024, 2048, 4096])
def test_new_inputs_see_the_nyquist_lines_and_single_edge_bins(n):
    """What the GPU tests would catch: a kernel that dropped the Nyquist column or row, or the single bin (0, 1) or (1, 0).  Each
    mutation is applied to xi and run through the oracle (JACOBIAN mode, t = 7.25); the largest change over the eight channels, as a
    fraction of the channel's max, is what a GPU test at 1e-5 sees.  Measured: lines >= 2.6e-2, single bins >= 3.3e-5 (white) and
    >= 2.6e-4 (edge)."""
    from oracle import oracle as O
    mutations = {"Nyquist column": (slice(None), 0), "Nyquist row": (0, slice(None)), "bin (0, 1)": (0, 1), "bin (1, 0)": (1, 0)}
    for family, make in (("white", S.white_xi), ("edge", S.edge_xi)):
        xi = make(n, 11)[0]
        _, base = oracle_frame(n, xi, O.MODE_JACOBIAN)
        for name, where in mutations.items():
            x = xi.copy()
            x[where] = 0.0
            _, mut = oracle_frame(n, x, O.MODE_JACOBIAN)
            moved = max(S.chan_err(mut, base))
            floor = 1e-3 if "Nyquist" in name else (1e-4 if family == "edge" else 1e-5)
            assert moved >= floor, (n, family, name, moved)
            del mut


@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_fp32_transforms_stay_at_the_float_floor_on_the_white_spectrum(n):
    """The oracle's fp32 FFT against its float64 FFT on a flat spectrum: <= 1e-6 of every channel's max (measured 2-3e-7), so the GPU
    tests' 1e-5 is as meaningful here as on a Phillips sea."""
    from oracle import oracle as O
    xi = S.white_xi(n, 5)[0]
    for mode in (O.MODE_FULL7, O.MODE_JACOBIAN):
        a64, f64 = oracle_frame(n, xi, mode)
        a32, f32 = oracle_frame(n, xi, mode, O.FFT_F32)
        assert abs(a32 - a64) <= 1e-6 * a64
        assert max(S.chan_err(f32, f64)) <= 1e-6, (n, mode, S.chan_err(f32, f64))
