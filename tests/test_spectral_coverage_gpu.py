"""Every spectrum bin through the kernels, Nyquist lines included (tests/spectra.py builds the inputs).

The rest of the suite feeds the kernels Phillips spectra, whose weakest lines are the Nyquist row and column (index 0 of each axis) --
exactly where the z pass has its special cases (ocean_kernels.h: the Nyquist column's Tx = S-, the parity rule of the Jacobian cross
derivative, the self-mirrored row N/2, the mirror indices of zpass_load_pair, the lone columns of the two-column form, the x passes'
half planes).  On those inputs a kernel that dropped the whole Nyquist column at 4096^2 would still meet 1e-5.  Here:

  * white and edge spectra (every bin, or every bin of the edge lines, at one amplitude) through every fp32 variant -- the store
    policies of test_variants_gpu.policies, depth 3, the merged x pass, the one-launch frame -- at 16 .. 4096, FULL7 and JACOBIAN,
    against the float64-FFT oracle at the suite's tolerances, each launch record checked to be the claimed variant;
  * a sparse spectrum (corners, Nyquist neighbours, mirror pairs, the DC bin) against a closed form that needs no FFT, in all four modes,
    t = 0, 7.25 and 3e5, serial and pipelined, at 16 .. 4096;
  * exhaustive impulses: N^2 tiles of N^2 texels in one launch for N = 16, 32, 64, tile i exciting bin i alone -- every bin and every
    mirror pairing of the small-tile code paths, each tile against the closed form;
  * the reduced-precision forms (half2 intermediates, fp16 spectrum) on the white and edge spectra: finite, and within 4x of the error
    measured on the MI355X (a flat spectrum is not a sea the 1e-3 Phillips contract describes): 2.7-4.2e-4 for half2, 2.4-2.8e-4 for
    the fp16 spectrum at 256 .. 4096.

Tolerances: per channel max|err| <= 1e-5 * max|channel|, amplitude / min / max 1e-6 of A (tests/test_parity_gpu.py).  A failure
names the bins that carry the residual (spectra.worst_bins).
"""
import hashlib

import numpy as np
import pytest

import spectra as S
from test_variants_gpu import handoff_grid_fits, policies

pytestmark = pytest.mark.gpu

TOL, TOL_AMP = 1e-5, 1e-6
FLOOR = 1e-7             # single-bin tiles: absolute error floor, as a fraction of the tile's largest field (test_every_single_bin_as_its_own_tile)
T = 7.25
SEED = 0x5EC70000
SIZES = [16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
FULL7, JACOBIAN = 0, 3
FAMILIES = {"white": S.white_xi, "edge": S.edge_xi}


class OracleFrames:
    """FFT_F64 oracle frames per (n, mode, the tile's xi); entries of other tile sizes are dropped when a new size comes (4096^2: 512 MB
    a frame)."""

    def __init__(self):
        self.n, self.frames = None, {}

    def get(self, n, xi, mode):
        from oracle import oracle as O
        if n != self.n:
            self.n, self.frames = n, {}
        key = (mode, hashlib.sha1(np.ascontiguousarray(xi).tobytes()).hexdigest())
        if key not in self.frames:
            o = S.make_oracle(n, xi)
            a, d, q = o.compute_waves(T, mode=mode, fft=O.FFT_F64)
            self.frames[key] = (a, d, q, o.min_height, o.max_height)
        return self.frames[key]


@pytest.fixture(scope="module")
def oracle_frames():
    return OracleFrames()


def new_batch(n, tiles, mode, depth=1, merged=True, inter_bits=32, h0_bits=32):
    import watersurfacerendering_amd as W
    b = W.OceanBatch(n, tiles, 0)
    b.set_params(**S.gpu_params())
    b.set_mode(mode)
    b.set_pipeline_depth(depth)
    b.set_merged_xpass(merged)
    b.set_intermediate_precision(inter_bits)
    b.set_spectrum_precision(h0_bits)
    return b


def frame(b, t, depth):
    """One frame at t; pipelined contexts run it behind frames in flight on the other chains."""
    if depth > 1:
        for j in range(depth - 1):
            b.compute_waves_async(0.3 * (j + 1))
        b.compute_waves_async(t)
        b.synchronize()
    else:
        b.compute_waves(t)


def check(d, q, h, ref, what, tol=TOL, tol_amp=TOL_AMP, jac=None):
    """Maps and heights of one tile against (A, disp, nrm, min, max) of the oracle or the closed form."""
    a, do, no, mn, mx = ref
    assert np.all(np.isfinite(d)) and np.all(np.isfinite(q)), what
    assert abs(h[0] - a) <= tol_amp * abs(a), (what, "A", h[0], a)
    assert abs(h[1] - mn) <= tol_amp * abs(a) and abs(h[2] - mx) <= tol_amp * abs(a), (what, "min/max", h, mn, mx)
    ed, en = S.chan_err(d, do), S.chan_err(q, no)
    if max(ed + en) > tol:
        got, want = np.concatenate([d, q], -1), np.concatenate([do, no], -1)
        pytest.fail(f"{what}: displacement {ed}, normal {en}; residual by bin (channel, (row, column), share): {S.worst_bins(got, want)}")
    if jac is False:
        assert np.all(d[..., 3] == 1.0), what
    return max(ed + en)


# --------------------------------------------------------------------------------------------------------------------------------
# white and edge spectra through every fp32 variant

def variants(n):
    """(name, tiles, depth, merged) per tile size: the store policies of test_variants_gpu.policies, depth 3, and up to 512^2 the
    pipelined three-launch frame (merged x pass switched off) beside the merged / one-launch forms the policies reach."""
    out = [(name, min(tiles, 65535), depth, True) for name, tiles, depth in policies(n)]      # (16^2: the launch grid's 65535 tiles, still streamed)
    out.append(("depth3", 1, 3, True))
    if n <= 512:
        out.append(("unmerged", 1, 2, False))
    return out


CASES = [(n, fam, mode, v) for n in SIZES for fam in FAMILIES for mode in (FULL7, JACOBIAN) for v in variants(n)]


@pytest.mark.parametrize("n,family,mode,variant", CASES,
                         ids=[f"{n}-{f}-{S.MODES[m]}-{v[0]}" for n, f, m, v in CASES])
def test_white_and_edge_spectra_through_every_variant(n, family, mode, variant, oracle_frames):
    from watersurfacerendering_amd import _abi as A
    name, tiles, depth, merged = variant
    jac = mode == JACOBIAN
    # what the launcher must select (ocean_launch.h; test_variants_gpu.test_every_selectable_variant_meets_the_oracle)
    merged_form = merged and n <= (128 if depth == 1 else 512) and tiles == 1 and not jac
    one_form = merged and n <= 128 and tiles == 1 and depth > 1 and not jac
    if one_form and not handoff_grid_fits(n, one_launch=True):
        pytest.skip(f"this device cannot hold the one-launch grid of a {n}^2 tile (handoff_grid_fits)")
    if merged_form and not handoff_grid_fits(n):
        pytest.skip(f"this device cannot hold the merged x-pass grid of a {n}^2 tile (handoff_grid_fits)")
    xis = FAMILIES[family](n, SEED + n, tiles)
    b = new_batch(n, tiles, mode, depth, merged)
    b.prepare(SEED, xis)
    frame(b, T, depth)
    z, xb, xd = b.last_launch()
    what = (n, family, S.MODES[mode], name)
    assert z["tile_size"] == n and z["grid_y"] == tiles and z["mode"] == mode, what
    assert all(bool(li["flags"] & A.OCEAN_LAUNCH_ONE_LAUNCH) == one_form for li in (z, xb, xd)), (what, "one-launch frame")
    assert bool(xb["flags"] & A.OCEAN_LAUNCH_MERGED_X) == bool(xd["flags"] & A.OCEAN_LAUNCH_MERGED_X) == merged_form, (what, "merged x pass")
    assert all(bool(li["flags"] & A.OCEAN_LAUNCH_JACOBIAN) == jac for li in (z, xb, xd)), what
    if name in ("plain", "batch", "nts", "stream") and not one_form:
        single = n == 4096 or (name != "stream" and (n == 2048 or (n == 1024 and tiles >= 2)))
        assert bool(z["flags"] & A.OCEAN_LAUNCH_SINGLE_TRANSFORM) == single, (what, "single-transform z pass")
        assert bool(z["flags"] & A.OCEAN_LAUNCH_NT_INTER) == (name == "stream"), (what, "streamed intermediates")
    for i in sorted({0, tiles - 1}):
        d, q = b.read_maps(i, 1)
        err = check(d[0], q[0], b.heights(i), oracle_frames.get(n, xis[i], mode), what + (f"tile {i}",), jac=jac)
        print(f"fp32 {family} N={n} {S.MODES[mode]} {name} tile {i}: max error {err:.3e}")
        del d, q
    b.close()


# --------------------------------------------------------------------------------------------------------------------------------
# sparse spectrum against the closed form

@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=S.MODES)
@pytest.mark.parametrize("n", SIZES)
def test_sparse_spectrum_meets_the_closed_form(n, mode):
    """The corners (0, 0), (0, N-1), (N-1, 0), (N-1, N-1), the Nyquist lines' neighbours, the self-mirrored row and column, mirror
    pairs and the DC bin (which must add nothing) against the FFT-free closed form, serial and at depth 2."""
    xi = S.sparse_xi(n)
    sp = S.spectrum_of(S.make_oracle(n, xi[0]))
    lam = S.PARAMS["lam"]
    refs = {t: S.closed_form(sp, t, lam, mode) for t in (0.0, 7.25, 3e5)}
    for depth in (1, 2):
        b = new_batch(n, 1, mode, depth)
        b.prepare(SEED, xi)
        for t, ref in refs.items():
            frame(b, t, depth)
            d, q = b.read_maps()
            err = check(d[0], q[0], b.heights(0), ref, (n, S.MODES[mode], depth, t), jac=mode == JACOBIAN)
            print(f"fp32 sparse N={n} {S.MODES[mode]} depth {depth} t={t}: max error {err:.3e}")
        b.close()


# --------------------------------------------------------------------------------------------------------------------------------
# every bin on its own

def impulse_xi(n):
    """|h0| = AMP on every bin, with the phase that makes the bin's real wave 2 Re(h0 exp(i w T)) = 2 AMP at the checked time: a lone
    bin whose wave happened to be near a zero crossing would leave only the rounding of that cancellation to compare."""
    u = S.unit(n)
    o = S.make_oracle(n, np.ones((n, n, 2), np.float32))      # (held until its array is copied: omega is a view of the oracle's own memory)
    om = o.omega.astype(np.float32)
    wt = (om * np.float32(T)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(u >= S.AMP * S.CAP, S.AMP / u, 0.0)
    return np.stack([s * np.cos(wt), -s * np.sin(wt)], axis=-1).astype(np.float32)


@pytest.mark.parametrize("mode", [FULL7, JACOBIAN], ids=["full7", "jacobian"])
@pytest.mark.parametrize("n", [16, 32, 64])
def test_every_single_bin_as_its_own_tile(n, mode):
    """One launch of N^2 tiles; tile m * N + q excites bin (m, q) alone (impulse_xi) and is checked
    against the closed form of that bin.  A single bin leaves some channels identically zero -- the slopes of the bin (0, 0), whose real
    part vanishes, Dx of a bin with kx = 0 -- where a relative tolerance has no denominator: there the GPU channel must stay within 1e-6
    of the largest un-normalised field of the tile.  A channel far below the tile's largest field meets 1e-5 of its own max or FLOOR
    of that field: the kernels transform two fields as one complex sequence, so a channel's rounding follows its partner's size --
    measured on the MI355X, dxDx of the bins (0, N/2 - 1) at 32^2 and (0, N/2 - 2) at 64^2, 2500x and 600x below their partner dzDz,
    carried 1.2e-10 and 4.3e-10 (1-2 fp32 ulps of dzDz; 1.5e-5 and 2.7e-5 of their own max).  The DC tile (a xi the k = 0 rule must discard) is the zero-spectrum case exactly:
    A = FLT_MIN, height 0, w = 1, every other channel 0 (test_parity_gpu.test_zero_spectrum_minmax_quirk)."""
    tiles = n * n
    flat = impulse_xi(n)
    xis = np.zeros((tiles, n, n, 2), np.float32)
    rows, cols = np.divmod(np.arange(tiles), n)
    xis[np.arange(tiles), rows, cols] = flat[rows, cols]
    dc = (n // 2) * n + n // 2
    xis[dc, n // 2, n // 2] = (5.0, -3.0)
    sp = S.spectrum_of(S.make_oracle(n, flat))
    lam = S.PARAMS["lam"]
    b = new_batch(n, tiles, mode)
    b.prepare(SEED, xis)
    amps = b.compute_waves(T)
    d, q = b.read_maps()
    b_h = np.array([b.heights(i) for i in range(tiles)], np.float64)
    b.close()
    assert np.array_equal(b_h[:, 0], amps.astype(np.float64))
    zero_channels = exact_zero = 0
    for m in range(n):                       # one row of bins per step
        sl = slice(m * n, (m + 1) * n)
        a, do, no, mn, mx = S.impulse_maps(sp, rows[sl], cols[sl], T, lam, mode)
        raw = np.stack([a] + [np.abs(x).max(axis=(1, 2)) for x in (do[..., 0], do[..., 2], no[..., 0], no[..., 1], no[..., 2], no[..., 3])], -1)
        scale = raw.max(axis=1)                                              # largest un-normalised field of each tile
        h = b_h[sl]
        assert np.all(np.abs(h[:, 0] - a) <= TOL_AMP * a), (n, m, "A")
        assert np.all(np.abs(h[:, 1] - mn) <= TOL_AMP * a) and np.all(np.abs(h[:, 2] - mx) <= TOL_AMP * a), (n, m, "min/max")
        for got, ref, map_name in ((d[sl], do, "displacement"), (q[sl], no, "normal")):
            assert np.all(np.isfinite(got)), (n, m, map_name)
            err = np.abs(got.astype(np.float64) - ref).max(axis=(1, 2))     # [bin, channel]
            den = np.abs(ref).max(axis=(1, 2))
            zero = den <= 1e-12 * np.maximum(scale, S.FLT_MIN)[:, None]
            if map_name == "displacement":
                zero[:, 1] = den[:, 1] == 0                                   # the normalised height (0 only for the DC tile)
            zero_channels += int(zero.sum())
            exact_zero += int((zero & (err == 0)).sum())
            bad_rel = ~zero & (err > np.maximum(TOL * den, FLOOR * scale[:, None]))
            bad_zero = zero & (err > 1e-6 * scale[:, None])
            for j, c in zip(*np.nonzero(bad_rel | bad_zero)):
                pytest.fail(f"N={n} {S.MODES[mode]} bin ({m}, {cols[sl][j]}) {map_name} channel {c}: max|err| {err[j, c]:.3e}, "
                            f"max|ref| {den[j, c]:.3e}, tile scale {scale[j]:.3e}")
    dc_d, dc_q = d[dc], q[dc]
    tiny = S.FLT_MIN
    assert amps[dc] == tiny and b_h[dc, 2] == tiny and b_h[dc, 1] == 0.0
    assert np.all(dc_d[..., [0, 1, 2]] == 0.0) and np.all(dc_d[..., 3] == 1.0) and np.all(dc_q == 0.0)
    print(f"N={n} {S.MODES[mode]}: {zero_channels} identically-zero channels in the closed form, {exact_zero} of them exactly 0 on the GPU")


# --------------------------------------------------------------------------------------------------------------------------------
# reduced precision on flat spectra

# (form, family, n) -> max error measured on the MI355X.  No sqrt(N) growth (the looseness of the column-sum bound of k_inter_bounds):
# 256 -> 4096 moves half2 from 3.5e-4 to 4.2e-4 (white) and 2.7e-4 to 4.2e-4 (edge); the fp16 spectrum stays at 2.4-2.8e-4.
MEASURED16 = {("half2", "white", 256): 3.54e-4, ("half2", "white", 1024): 3.97e-4, ("half2", "white", 4096): 4.17e-4,
              ("half2", "edge", 256): 2.70e-4, ("half2", "edge", 1024): 3.20e-4, ("half2", "edge", 4096): 4.16e-4,
              ("fp16spectrum", "white", 256): 2.56e-4, ("fp16spectrum", "white", 1024): 2.61e-4, ("fp16spectrum", "white", 4096): 2.48e-4,
              ("fp16spectrum", "edge", 256): 2.47e-4, ("fp16spectrum", "edge", 1024): 2.37e-4, ("fp16spectrum", "edge", 4096): 2.77e-4}


@pytest.mark.parametrize("form", ["half2", "fp16spectrum"])
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("n", [256, 1024, 4096])
def test_reduced_precision_on_flat_spectra(n, family, form, oracle_frames):
    """half2 intermediates (ocean_set_intermediate_precision(16)) and the fp16 spectrum (ocean_set_spectrum_precision(16)) on the white
    and edge spectra, FULL7 and JACOBIAN.  Every value finite -- k_inter_bounds' overflow bound does not depend on the spectrum's shape --
    and the largest channel error (height, Dx, Dz, both slopes, dxDx, dzDz; the Jacobian in JACOBIAN mode) within 4x of MEASURED16."""
    bits = dict(inter_bits=16) if form == "half2" else dict(h0_bits=16)
    xis = FAMILIES[family](n, SEED + n, 1)
    worst = 0.0
    for mode in (FULL7, JACOBIAN):
        b = new_batch(n, 1, mode, **bits)
        b.prepare(SEED, xis)
        frame(b, T, 1)
        d, q = b.read_maps()
        h = b.heights(0)
        b.close()
        assert np.all(np.isfinite(d)) and np.all(np.isfinite(q)), (n, family, form, mode)
        a, do, no, mn, mx = oracle_frames.get(n, xis[0], mode)
        e = max(S.chan_err(d[0], do)[: 4 if mode == JACOBIAN else 3] + S.chan_err(q[0], no) + [abs(h[0] - a) / a])
        worst = max(worst, e)
    print(f"reduced precision {form} {family} N={n}: max error {worst:.3e}")
    bound = 4.0 * MEASURED16[(form, family, n)]
    assert TOL / 10 < worst <= bound, (n, family, form, worst, bound)
