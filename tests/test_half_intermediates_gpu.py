"""The half2 intermediates (ocean_set_intermediate_precision(16): store_z<..., Z16> / load_z<true> of every frame kernel, the scales of
k_inter_bounds and ocean_prepare) held to their own rounding.

The rest of the suite holds this mode to 1e-3 of each channel's maximum against the UNquantised oracle, two to five times its own
rounding noise: a Z16 kernel that rounded toward zero, swapped two scales or read a mirrored half with the wrong sign by a little
would pass.  Here every frame is compared with tests/half_intermediates.frame -- the float64 two-pass transform that rounds the z-pass
outputs to the same halves, fed the device's own h0 and omega -- and must lie much nearer to it than the rounding is large:

    rms(gpu - restated) <= RHO * rms(restated - oracle)      per channel
    max|gpu - restated| <= max|restated - oracle|            per channel (a half rounded the other way costs no more than a rounding)
    |A_gpu - A_restated| <= 1e-5 A                           (A is the maximum of a quantised map here)
    every value finite; the frame within Z16_TOL = 1e-3 of the unquantised oracle and further than TOL / 10 = 1e-6 from it

What remains between a frame and the restatement is the fp32 arithmetic of the z pass (1e-7 of a column) and the halves it rounds the
other way; a different rounding mode or an independent quantisation gives an rms ratio of 1.3 and more (tests/test_half_intermediates.py
measures that on the CPU), so RHO, at most 0.5, keeps a factor of two on that side.  The scales are restated, not read back: every case
asserts on its own spectrum that each quotient a scale is taken from is further than 1e-3 from a power of two, which the order of an
fp32 sum cannot bridge.

Cases: the z-pass code paths tests/test_variants_gpu.py names (FORMS below is asserted to be that set), per-tile scales, alternative
parameters, pipelined frames, the fp16 spectrum beside the half2 intermediates, a JONSWAP tile, white and edge-line spectra (the Nyquist
row and column, the `keeps` rule and the self-mirrored units carry weight there), a velocity twin, and the aligned frame -- draws
(1, 0) at t = 0: every h0 real and non-negative, the height's row 0 of the heaviest column is that column's sum plus its mirror's, the
stored halves reach 4096 and more, and a scale 8 times too large overflows.

MEASURED: the worst channel's rms ratio of every case on an MI355X (frames are bit-reproducible: one number each); RHO is twice the
worst of them.
"""
import numpy as np
import pytest

import empirical_spectra as E
import half_intermediates as HI
import half_maps as H
import spectra as S
import velocity as V

pytestmark = pytest.mark.gpu

TOL, Z16_TOL, TOL_AMP_Q = 1e-5, 1e-3, 1e-5      # tests/test_parity_gpu.py: TOL, Z16_TOL; A against the restatement
DISTANCE = 1e-3                                   # every scale's quotient is at least this far from a power of two
SEED = 0x5EED1600
ALT = dict(length=250.0, wind=(1.0, 0.0), wind_speed=10.0, lam=-2.0)          # = tests/test_parity_gpu.ALT (asserted below)
ST = 128                                          # OCEAN_LAUNCH_SINGLE_TRANSFORM (asserted below)

# worst channel's rms(gpu - restated) / rms(restated - oracle) per case, measured on an MI355X (every case prints its own, with the
# worst max ratio -- 0.60 over the module, at 2048^2 -- and the error of A -- 9.0e-6 for the white spectrum at 256^2 in the Jacobian
# mode, where a flat spectrum leaves several near-equal extrema; below 1.6e-6 everywhere else)
MEASURED = {
    "default 16 full7 t 0": 0.0095, "default 16 full7 t 4.5": 0.1002, "default 16 jacobian t 0": 0.0095,
    "default 16 jacobian t 4.5": 0.1002, "default 64 full7 t 0": 0.0571, "default 64 full7 t 4.5": 0.1326,
    "default 64 jacobian t 0": 0.0571, "default 64 jacobian t 4.5": 0.1326, "default 256 full7 t 0": 0.0886,
    "default 256 full7 t 4.5": 0.0644, "default 256 jacobian t 0": 0.1320, "default 256 jacobian t 4.5": 0.0644,
    "default 512 full7 t 0": 0.0376, "default 512 full7 t 4.5": 0.0482, "default 512 jacobian t 0": 0.0376,
    "default 512 jacobian t 4.5": 0.0482, "default 1024 full7 t 0": 0.0615, "default 1024 full7 t 4.5": 0.0433,
    "default 1024 jacobian t 0": 0.0615, "default 1024 jacobian t 4.5": 0.0433, "batch 2 x 1024 full7 tile 0 t 4.5": 0.0433,
    "batch 2 x 1024 full7 tile 1 t 4.5": 0.0457, "default 2048 full7 t 4.5": 0.0673, "default 4096 full7 t 4.5": 0.0606,
    "stream 16 x 1024 full7 tile 0 t 4.5": 0.0433, "stream 16 x 1024 full7 tile 7 t 4.5": 0.0696,
    "per-tile 3 x 64 full7 tile 0 t 4.5": 0.0148, "per-tile 3 x 64 full7 tile 1 t 4.5": 0.0162,
    "per-tile 3 x 64 full7 tile 2 t 4.5": 0.0364, "per-tile 3 x 64 jacobian tile 0 t 4.5": 0.0283,
    "per-tile 3 x 64 jacobian tile 1 t 4.5": 0.0162, "per-tile 3 x 64 jacobian tile 2 t 4.5": 0.0364, "alt 512 full7 t 4.5": 0.0670,
    "alt 512 jacobian t 4.5": 0.0670, "depth 3 256 full7 t 4.5": 0.0454, "fp16 spectrum 64 full7 t 4.5": 0.0669,
    "fp16 spectrum 512 full7 t 4.5": 0.0690, "jonswap 64 full7 t 4.5": 0.1322, "white 64 full7 t 4.5": 0.0424,
    "white 64 jacobian t 4.5": 0.0424, "white 256 full7 t 4.5": 0.0750, "white 256 jacobian t 4.5": 0.0750,
    "edge 64 full7 t 4.5": 0.0664, "edge 64 jacobian t 4.5": 0.0664, "edge 256 full7 t 4.5": 0.0771, "edge 256 jacobian t 4.5": 0.0771,
    "aligned 64 full7 t 0": 0.0464, "aligned 64 jacobian t 0": 0.0464, "aligned 512 full7 t 0": 0.0590,
    "aligned 512 jacobian t 0": 0.0508, "twin 64 full7 tile 0 t 4.5": 0.0172, "twin 64 full7 tile 1 t 4.5": 0.0106,
}
RHO = min(0.5, 2.0 * max(MEASURED.values()))      # 0.2652: twice the worst (the default sea at 64^2, t = 4.5)
LAUNCHED = set()                                  # (tile size, z-pass flags, columns per workgroup) of every frame this run launched
SEEN = {}                                         # what this run measured: case -> (rms ratio, max ratio, A error), printed per case


# --------------------------------------------------------------------------------------------------------------------------------
# inputs: what a tile is prepared from, on the device and in numpy

def sea(**kw):
    """Oracle-style parameters (oracle.DEFAULTS patched)."""
    from oracle import oracle as O
    return dict(O.DEFAULTS, **kw)


def gpu_params(p):
    return dict(tile_length=p["length"], wind_dir_x=p["wind"][0], wind_dir_y=p["wind"][1], wind_speed=p["wind_speed"],
                anim_period=p["anim_period"], phillips_const=p["phillips_a"], damping=p["damping"], lambda_=p["lam"])


def draws(n, kind, seed):
    from oracle import oracle as O
    if kind == "gauss":
        return O.gauss_xi_numpy(seed, n)
    if kind == "aligned":
        xi = np.zeros((n, n, 2), np.float32)
        xi[..., 0] = 1.0
        return xi
    return {"white": S.white_xi, "edge": S.edge_xi}[kind](n, seed)[0]


def tile(n, kind="gauss", seed=SEED, spec=None, twin_of=None, **params):
    """One tile's input: tile size, draws, parameters, an empirical spectrum (or None), the tile it is the velocity twin of (or None)."""
    p = dict(S.PARAMS) if kind in ("white", "edge") and not params else sea(**params)
    return dict(n=n, kind=kind, seed=seed, params=p, spec=spec, twin_of=twin_of)


def numpy_prep(tl, xi, h0=None, omega=None, h16=False):
    """oracle.numpy_prepare's dictionary of a tile; h0 and omega the device's where given, else restated; h16: the fp16 copy."""
    from oracle import oracle as O
    p = tl["params"]
    prep = O.numpy_prepare(tl["n"], xi, **p)
    if h0 is not None:
        prep["h0"], prep["omega"] = V.as_complex(h0), np.asarray(omega, np.float32)
    else:
        if tl["spec"] is not None:
            prep["h0"] = E.restate_h0(prep, xi, tl["spec"], length=p["length"], wind=p["wind"], wind_speed=p["wind_speed"])
        if tl["twin_of"] is not None:
            prep["h0"] = V.as_complex(V.derive_spectrum(prep["h0"], prep["omega"]))
    if h16:
        prep["h0_fp32"] = prep["h0"]
        prep["h0"] = V.as_complex(H.quantise_h0(np.stack([prep["h0"].real, prep["h0"].imag], axis=-1)))
    return prep


# --------------------------------------------------------------------------------------------------------------------------------
# one frame, and the criterion

def run(tiles, jac, times, depth=1, h16=False):
    """A context of `tiles` with half2 intermediates; one frame per entry of `times`, each behind depth - 1 asynchronous frames.  Yields
    (t, launches, read), read(i) -> (disp, nrm, heights, numpy_prep of the device's own spectrum) of tile i."""
    import watersurfacerendering_amd as W
    from watersurfacerendering_amd import _abi as A
    assert A.OCEAN_LAUNCH_SINGLE_TRANSFORM == ST
    n = tiles[0]["n"]
    b = W.OceanBatch(n, len(tiles), 0)
    try:
        xi = np.stack([draws(n, tl["kind"], tl["seed"]) for tl in tiles])
        for i, tl in enumerate(tiles):
            if tl["twin_of"] is not None:
                b.set_velocity_twin(i, tl["twin_of"])
        for i, tl in enumerate(tiles):
            if tl["twin_of"] is None:
                b.set_params(tile=i, **gpu_params(tl["params"]))
                if tl["spec"] is not None:
                    b.set_spectrum(i, **tl["spec"])
        b.set_intermediate_precision(16)
        b.set_spectrum_precision(16 if h16 else 32)
        b.set_mode(A.OCEAN_MODE_JACOBIAN if jac else A.OCEAN_MODE_FULL7)
        b.set_pipeline_depth(depth)
        b.prepare(0, xi)
        for t in times:
            if depth > 1:
                for j in range(depth - 1):
                    b.compute_waves_async(0.3 * (j + 1))
                b.compute_waves_async(t)
                b.synchronize()
            else:
                b.compute_waves(t)
            launches = b.last_launch()
            LAUNCHED.add((n, launches[0]["flags"], launches[0]["per_workgroup"]))
            z = launches[0]
            assert z["tile_size"] == n and z["grid_y"] == len(tiles) and bool(z["flags"] & A.OCEAN_LAUNCH_FP16_SPECTRUM) == h16, z
            for li in launches:
                assert li["flags"] & A.OCEAN_LAUNCH_HALF_INTER and bool(li["flags"] & A.OCEAN_LAUNCH_JACOBIAN) == jac, li

            def read(i):
                d, q = b.read_maps(i, 1)
                h0, om = b.read_spectrum(i)
                src = tiles[i]["twin_of"] if tiles[i]["twin_of"] is not None else i
                assert np.array_equal(b.read_xi(src), xi[src])
                return d[0], q[0], b.heights(i), numpy_prep(tiles[i], xi[src], h0, om, h16)

            yield t, launches, read
    finally:
        b.close()


def form(launches):
    """(single-transform batches?, spectrum columns per workgroup) of the z pass that ran."""
    z = launches[0]
    return (bool(z["flags"] & ST), z["per_workgroup"])


def references(prep, t, lam, jac, info):
    """(restated frame, unquantised oracle).  Up to 1024^2 the oracle is oracle.numpy_compute_waves; beyond, the restatement's own two
    passes without the rounding, off the same first-axis transforms (tests/test_half_intermediates.py holds the two together to 1e-12)."""
    from oracle import oracle as O
    if prep["kx"].shape[0] <= 1024:
        return HI.frame(prep, t, lam, jac, info=info), O.numpy_compute_waves(prep, t, lam=lam, jacobian=jac)
    return HI.frame_pair(prep, t, lam, jac, info=info)


def holds(case, d, q, h, prep, t, lam, jac, stored_at_least=None):
    """The criterion of the module's docstring for one tile of one frame."""
    assert case in MEASURED, case                # a new case brings its measured figure
    info = {}
    restated, oracle = references(prep, t, lam, jac, info)
    sc = info["scales"]
    assert min(sc["distance"].values()) > DISTANCE, (case, sc)
    if "h0_fp32" in prep:                        # k_inter_bounds sums the fp32 spectrum, the restatement its fp16 copy: the same choices
        sc32 = HI.scales(prep["h0_fp32"], prep["kx"], prep["kz"])
        assert all(sc32[k] == sc[k] for k in ("su", "sk", "g", "s3")) and min(sc32["distance"].values()) > DISTANCE, (case, sc, sc32)
    if stored_at_least is not None:
        assert info["max_scaled"] >= stored_at_least, (case, info["max_scaled"])
    assert np.all(np.isfinite(d)) and np.all(np.isfinite(q)), case
    g, r, o = HI.channels(d, q), HI.channels(restated[1], restated[2]), HI.channels(oracle[1], oracle[2])
    rat = HI.ratios(g, r, o)
    for c, (rr, _) in enumerate(rat):
        if rr is None:                           # nothing was rounded in this channel (FULL7's constant w = 1): the same values
            assert np.array_equal(g[c], r[c]), (case, c)
    rms = [x for x, _ in rat if x is not None]
    mx = [x for _, x in rat if x is not None]
    assert len(rms) == (8 if jac else 7), (case, rat)                       # every channel but FULL7's constant w carries a rounding
    a_err = abs(h[0] - restated[0]) / restated[0]
    err_u = HI.errors(g, o)
    err_q = HI.errors(g, r)
    SEEN[case] = (max(rms), max(mx), a_err)
    print(f"half2 {case}: rms ratio {max(rms):.4f} max ratio {max(mx):.4f} A {a_err:.2e} | worst channel against the restatement "
          f"{max(err_q):.2e}, against the oracle {max(err_u):.2e} | su {sc['su']:g} sk {sc['sk']:g} s3 {sc['s3']:g} g {sc['g']:g} "
          f"largest stored {info['max_scaled']:.0f}")
    assert max(rms) <= RHO, (case, "rms", rat)
    assert max(mx) <= 1.0, (case, "max", rat)
    assert a_err <= TOL_AMP_Q, (case, h[0], restated[0])
    assert abs(h[0] - oracle[0]) <= Z16_TOL * oracle[0], (case, h[0], oracle[0])
    assert TOL / 10 < max(err_u) and max(err_u) <= Z16_TOL, (case, err_u)
    return sc


def frames(case, tiles, jac, times, check=None, depth=1, h16=False, want_form=None, stored_at_least=None):
    """Runs the context and holds tiles `check` (default: all) of every frame to the criterion; returns the scales per checked tile."""
    out = {}
    for t, launches, read in run(tiles, jac, times, depth, h16):
        if want_form is not None:
            assert form(launches) == want_form, (case, launches[0])
        for i in (range(len(tiles)) if check is None else check):
            d, q, h, prep = read(i)
            src = tiles[i]["twin_of"] if tiles[i]["twin_of"] is not None else i
            out[i] = holds(f"{case} tile {i} t {t:g}" if len(tiles) > 1 else f"{case} t {t:g}", d, q, h, prep, t, tiles[src]["params"]["lam"],
                           jac, stored_at_least)
    return out


def mode_name(jac):
    return "jacobian" if jac else "full7"


# --------------------------------------------------------------------------------------------------------------------------------
# the z-pass code paths

# (n, the z-pass form a lone tile takes): two-transform batches at 16 and 64, four-transform batches at 256 and 512, the lone-tile
# (two-transform) form at 1024
LONE = [(16, (False, 1)), (64, (False, 1)), (256, (False, 1)), (512, (False, 1)), (1024, (False, 1))]
BATCH_1024, STREAM_1024, BIG = (1024, (True, 1)), (1024, (False, 2)), [(2048, (True, 1)), (4096, (True, 1))]
STREAM_2048 = (2048, (False, 2))
FORMS = {(n, f) for n, f in LONE + [BATCH_1024, STREAM_1024, STREAM_2048] + BIG if n >= 64}


def test_the_cases_cover_every_z16_zpass_form_the_variants_test_enumerates():
    """tests/test_variants_gpu.expected_variants: per tile size, every (z-pass flags, columns per workgroup) the launcher can select.
    Of those with half2 intermediates, the z-pass FORMS -- single-transform batches or not, one or two columns; the two- and
    four-transform batches go with the tile size -- must be the ones this module's cases declare (each case asserts that its form ran;
    test_zz_every_declared_form_was_launched asserts it once more on what the module's frames reported).

    What a form is here: the SINGLE_TRANSFORM bit and the columns per workgroup, i.e. the kernel bodies that compute and place the
    values.  The store policy of the intermediates (NT_INTER: store_z<ZNT = true, Z16>, the same conversion and the same address, a
    non-temporal store) is not part of it: it is driven at 1024^2 and 2048^2, where the two-column form needs it, not at the other
    sizes nor at 4096^2 in flight; for those this module leans on tests/test_variants_gpu.py, which holds every store policy of one
    configuration to the same bits.  The 2048^2 two-column form is held by that same bit-equality with the lone tile's frame, not by
    a restatement of its own (test_large_tiles)."""
    import test_parity_gpu as P
    import test_variants_gpu as VG
    from watersurfacerendering_amd import _abi as A
    assert P.ALT == ALT and P.Z16_TOL == Z16_TOL and P.TOL == TOL and VG.TOL16 == Z16_TOL
    want = {(n, (bool(zf & ST), zw)) for size in (64, 256, 512, 1024, 2048, 4096) for n, zf, zw, _, _ in VG.expected_variants(size)
            if zf & A.OCEAN_LAUNCH_HALF_INTER}
    assert FORMS == want, {"not driven here": sorted(want - FORMS), "not enumerated there": sorted(FORMS - want)}
    assert ("stream", 16, 2) in VG.policies(1024) and ("stream", 4, 2) in VG.policies(2048)      # the smallest triggers of the two-column form


@pytest.mark.parametrize("jac", [False, True], ids=mode_name)
@pytest.mark.parametrize("n,want", LONE, ids=[str(n) for n, _ in LONE])
def test_default_sea(n, want, jac):
    frames(f"default {n} {mode_name(jac)}", [tile(n)], jac, (0.0, 4.5), want_form=want)


def test_batch_of_two_1024_tiles_takes_the_single_transform_form():
    n, want = BATCH_1024
    frames(f"batch 2 x {n} full7", [tile(n, seed=SEED + i) for i in range(2)], False, (4.5,), want_form=want)


@pytest.mark.parametrize("n,want", BIG, ids=[str(n) for n, _ in BIG])
def test_large_tiles(n, want):
    """One FULL7 frame at t = 4.5.  At 2048^2 the streamed two-column form too -- four tiles at depth 2, its smallest trigger -- whose
    tile 0 must be the lone tile's frame bit for bit (store policies and z-pass forms never change a bit: tests/test_variants_gpu.py),
    so that the criterion just met holds for it as it stands."""
    lone = None
    for t, launches, read in run([tile(n)], False, (4.5,)):
        assert form(launches) == want, launches[0]
        d, q, h, prep = read(0)
        holds(f"default {n} full7 t {t:g}", d, q, h, prep, t, -1.0, False)
        lone = (d, q, h)
    if n == STREAM_2048[0]:
        for t, launches, read in run([tile(n, seed=SEED + i) for i in range(4)], False, (4.5,), depth=2):
            assert form(launches) == STREAM_2048[1], launches[0]
            d, q, h, _ = read(0)
            assert np.array_equal(d, lone[0]) and np.array_equal(q, lone[1]) and h == lone[2]


def test_streamed_two_column_form_at_its_smallest_trigger():
    """16 x 1024^2 at depth 2 (tests/test_variants_gpu.policies(1024): "stream"); tiles 0 and 7 are restated."""
    n, want = STREAM_1024
    frames(f"stream 16 x {n} full7", [tile(n, seed=SEED + i) for i in range(16)], False, (4.5,), check=(0, 7), depth=2, want_form=want)


# --------------------------------------------------------------------------------------------------------------------------------
# scales, parameters, pipelining, the other reduced precision, other spectra

PER_TILE = [dict(length=1000.0, wind=(1.0, 1.0), phillips_a=3e-7), dict(length=370.0, wind=(1.0, -0.3), phillips_a=3e-5),
            dict(length=93.0, wind=(-0.2, 1.0), wind_speed=12.0, phillips_a=3e-7)]


def per_tile_tiles():
    return [tile(64, seed=SEED + 40 + i, **p) for i, p in enumerate(PER_TILE)]


def test_every_tile_of_a_batch_is_stored_with_its_own_scales():
    """Three tiles whose scales differ (su 512 / 256 / 32768, sk 16384 / 8192 / 131072).  What this can tell: a power of two applied in
    store and load alike leaves every half the same bits unless something overflows or goes subnormal, so a tile stored with ANOTHER
    tile's scales is noticed only in the direction "far too large" -- tile 2's scales on tiles 0 or 1 overflow (64 and 128 times theirs);
    tiles 0 and 1 exchanged, or too small a scale anywhere, change nothing.  A store and a load that disagree on the tile are noticed
    in every direction."""
    pre = [HI.scales(p["h0"], p["kx"], p["kz"]) for p in (numpy_prep(tl, draws(64, tl["kind"], tl["seed"])) for tl in per_tile_tiles())]
    assert len({s["su"] for s in pre}) > 1 and len({s["sk"] for s in pre}) > 1, pre           # there are scales to mix up
    sc = frames("per-tile 3 x 64 full7", per_tile_tiles(), False, (4.5,))
    assert len({s["su"] for s in sc.values()}) > 1 and len({s["sk"] for s in sc.values()}) > 1, sc
    sc = frames("per-tile 3 x 64 jacobian", per_tile_tiles(), True, (4.5,))
    assert len({s["s3"] for s in sc.values()}) > 1, sc


@pytest.mark.parametrize("jac", [False, True], ids=mode_name)
def test_alternative_parameters(jac):
    frames(f"alt 512 {mode_name(jac)}", [tile(512, seed=SEED + 1, **ALT)], jac, (4.5,))


def test_third_of_three_frames_in_flight():
    frames("depth 3 256 full7", [tile(256, seed=SEED + 12)], False, (4.5,), depth=3)


@pytest.mark.parametrize("n", [64, 512])
def test_fp16_spectrum_beside_the_half2_intermediates(n):
    """Both reduced precisions at once: the restatement is fed tests/half_maps.quantise_h0 of the device's h0 (and takes its
    scales from it; `holds` asserts that the fp32 spectrum, which k_inter_bounds sums, gives the same ones)."""
    frames(f"fp16 spectrum {n} full7", [tile(n, seed=SEED + 3)], False, (4.5,), h16=True)


JONSWAP = dict(length=500.0, wind=(1.0, 0.4142135), wind_speed=10.0)


def jonswap_tile():
    return tile(64, seed=SEED + 4, spec=E.spectrum(kind=E.JONSWAP, spreading=E.HASSELMANN), **JONSWAP)


def test_jonswap_tile():
    frames("jonswap 64 full7", [jonswap_tile()], False, (4.5,))


@pytest.mark.parametrize("jac", [False, True], ids=mode_name)
@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("family", ["white", "edge"])
def test_nyquist_lines_carry_weight(family, n, jac):
    """Flat spectra put weight on the Nyquist row and column, the `keeps` rule and the self-mirrored units.  They are NOT a check of the
    pair-to-scale mapping `c == 0 ? su : sk`: |h0| is constant, and at 256^2 the restated scales are su == sk == 2048 with g == 1, so a
    kernel that swapped the two passes those four cases (at 64^2 they differ: 8192 and 32768).  The Phillips, ALT, pipelined,
    fp16-spectrum and aligned cases at 256^2 and 512^2 are what holds the mapping of the four-transform form."""
    frames(f"{family} {n} {mode_name(jac)}", [tile(n, kind=family, seed=SEED + 5)], jac, (4.5,))


@pytest.mark.parametrize("jac", [False, True], ids=mode_name)
@pytest.mark.parametrize("n", [64, 512])
def test_aligned_frame_comes_near_the_top_of_the_format(n, jac):
    """Draws (1, 0): at t = 0 every h~ is real, non-negative and as large as it gets, so the stored halves come as near the top of the
    format as the bound's factor of 4 lets any frame come (4096 and more of 65504); a scale 8 times too large overflows here.  Finite
    at t = 4.5 too."""
    frames(f"aligned {n} {mode_name(jac)}", [tile(n, kind="aligned")], jac, (0.0,), stored_at_least=4096.0)
    for t, _, read in run([tile(n, kind="aligned")], jac, (4.5,)):
        d, q, h, _ = read(0)
        assert np.all(np.isfinite(d)) and np.all(np.isfinite(q)) and np.all(np.isfinite(h)), (n, jac, t)


def twin_tiles():
    return [tile(64, seed=SEED + 6), tile(64, seed=SEED + 6, twin_of=0)]


def test_velocity_twin_is_stored_with_the_bounds_of_its_own_spectrum():
    """The twin's spectrum i w h0 is weighted to high k: other bounds, and other scales than its source's (su 1024 against 512, s3 512
    against 256, sk 16384 both).  As in the per-tile batch, the criterion holds the twin to its own frame and to a store and a load that
    agree; it cannot tell a twin stored AND loaded with its source's scales, a factor of two that overflows nothing here."""
    sc = frames("twin 64 full7", twin_tiles(), False, (4.5,))
    assert sc[0]["su"] != sc[1]["su"] and sc[0]["s3"] != sc[1]["s3"] and sc[1]["b0"] > 0, sc


# --------------------------------------------------------------------------------------------------------------------------------

def all_inputs():
    """(name, tile, h16) of every spectrum this module prepares: tests/test_half_intermediates.py asserts the distance condition on the
    numpy restatement of each, without a device."""
    out = [(f"default {n}", tile(n), False) for n, _ in LONE + BIG]
    out += [(f"batch 1024 tile {i}", tile(1024, seed=SEED + i), False) for i in range(2)]
    out += [(f"stream 1024 tile {i}", tile(1024, seed=SEED + i), False) for i in (0, 7)]
    out += [(f"per-tile {i}", tl, False) for i, tl in enumerate(per_tile_tiles())]
    out += [("alt 512", tile(512, seed=SEED + 1, **ALT), False), ("depth 3 256", tile(256, seed=SEED + 12), False)]
    out += [(f"fp16 spectrum {n}", tile(n, seed=SEED + 3), True) for n in (64, 512)]
    out += [("jonswap 64", jonswap_tile(), False)]
    out += [(f"{fam} {n}", tile(n, kind=fam, seed=SEED + 5), False) for fam in ("white", "edge") for n in (64, 256)]
    out += [(f"aligned {n}", tile(n, kind="aligned"), False) for n in (64, 512)]
    out += [(f"twin tile {i}", tl, False) for i, tl in enumerate(twin_tiles())]
    return out


def test_zz_every_declared_form_was_launched():
    """Last in the module: (n, flags, per_workgroup) of every z pass the cases above launched, collected from ocean_last_launch, reduced
    to the form as in the first test, is the declared set -- and every one of them carried OCEAN_LAUNCH_HALF_INTER.  (Needs the whole
    module to have run.)"""
    from watersurfacerendering_amd import _abi as A
    got = {(n, (bool(f & ST), zw)) for n, f, zw in LAUNCHED if n >= 64}
    hint = ("this test reads what the module's other tests launched in THIS process: run the whole module "
            "(pytest tests/test_half_intermediates_gpu.py), not this test alone, with -k, or spread over workers")
    assert got == FORMS, {"declared, never launched here": sorted(FORMS - got), "launched, not declared": sorted(got - FORMS), "note": hint}
    assert all(f & A.OCEAN_LAUNCH_HALF_INTER for _, f, _ in LAUNCHED), sorted(LAUNCHED)
    assert any(f & A.OCEAN_LAUNCH_NT_INTER for _, f, _ in LAUNCHED)                 # the streamed store of the halves ran too
