"""The Gerstner proxy on the MI355X (ocean_extract_waves, ocean_set_waves / ocean_get_waves, ocean_eval_waves, ocean_query_waves and their
device forms) against tests/waves.py: the extraction bit for bit in every field and in the energy, the evaluation within twice the derived
bound per output channel, the proxy against the frame's own maps, the Newton inverse, readiness and errors.  Largest error / bound ratios
seen on the device (forward evaluation, over every case of test_evaluation_*): see the docstring of test_evaluation_within_the_bound."""
import ctypes as C

import numpy as np
import pytest

import spectra as SPC
import waves as WV

pytestmark = pytest.mark.gpu
f32 = np.float32
E_INVALID, E_NOT_READY = -1, -4
GENTLE = dict(wind_dir_x=1.0, wind_dir_y=0.4142135, wind_speed=30.0, anim_period=200.0, phillips_const=5e-11, damping=0.1, lambda_=-1.0)
SCALES8 = (1.0, 1.37, 2.11, 0.73, 3.3, 0.31, 5.1, 1.9)
KS = (1, 2, 63, 64, 65, 256, 1000, 4096)


def W():
    import watersurfacerendering_amd as w
    return w


def same_rows(got, want, what):
    assert got.dtype == WV.WAVE_DTYPE and len(got) == len(want), (what, len(got), len(want))
    g, w = got.view(np.uint32).reshape(len(got), 12), np.ascontiguousarray(want).view(np.uint32).reshape(len(want), 12)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert bad.size == 0, (what, int(bad[0]), got[bad[0]], want[bad[0]])


def check_extraction(b, tile, k, length, what):
    h0, om = b.read_spectrum(tile)
    want, energy = WV.extract(h0, om, length, k)
    rows, e = b.extract_waves(k, tile)
    same_rows(rows, want, what)
    assert np.float64(e).tobytes() == np.float64(energy).tobytes(), (what, e, energy)
    return rows


@pytest.mark.parametrize("n", [16, 64, 256, 1024])
def test_extraction_bit_for_bit(n):
    b = W().OceanBatch(n, 1)
    b.prepare(seed=0x5EED0000 + n)
    for k in KS:
        rows = check_extraction(b, 0, k, 1000.0, f"N={n} K={k}")
        again, _ = b.extract_waves(k, 0)
        assert rows.tobytes() == again.tobytes(), (n, k)
        assert b.get_waves(0).tobytes() == rows.tobytes(), (n, k)
    b.close()


def test_extraction_at_2048():
    b = W().OceanBatch(2048, 1)
    b.prepare(seed=0x5EED2048)
    check_extraction(b, 0, 256, 1000.0, "N=2048 K=256")
    b.close()


def test_extraction_of_a_sparse_sea_lists_every_excited_bin():
    n = 64
    b = W().OceanBatch(n, 1)
    b.set_params(**SPC.gpu_params())
    b.prepare(xi=SPC.sparse_xi(n))
    rows = check_extraction(b, 0, 64, SPC.PARAMS["length"], "sparse")
    excited = {m * n + q for m, q in SPC.sparse_bins(n) if (m, q) != (n // 2, n // 2)}
    assert set(int(x) for x in rows["bin"]) == excited and len(rows) == len(excited)
    b.close()


def test_extraction_inside_a_batch_with_per_tile_parameters_and_a_twin():
    n = 64
    b = W().OceanBatch(n, 4)
    lengths = (1000.0, 613.0, 250.0)
    for i, L in enumerate(lengths):
        b.set_params(i, tile_length=L, wind_speed=20.0 + 5 * i, wind_dir_x=1.0, wind_dir_y=0.3 * i)
    b.set_velocity_twin(3, 1)
    b.prepare(seed=77)
    for tile, L in ((1, lengths[1]), (2, lengths[2]), (3, lengths[1])):       # the twin lists its derivative spectrum on its source's lattice
        check_extraction(b, tile, 100, L, f"tile {tile}")
    h1, om1 = b.read_spectrum(1)
    h3, _ = b.read_spectrum(3)
    assert np.array_equal(h3[..., 0], -(om1 * h1[..., 1])) and np.array_equal(h3[..., 1], om1 * h1[..., 0])
    assert len(b.get_waves(1)) == 100 and len(b.get_waves(3)) == 100
    with pytest.raises(W().OceanError) as e:
        b.get_waves(0)
    assert e.value.code == E_NOT_READY
    b.close()


def mirrored_xi(n, seed=3):
    from oracle import oracle as O
    xi = O.gauss_xi_numpy(seed, n)
    idx = (n - np.arange(n)) % n
    sym = xi.copy()
    upper = np.arange(n * n).reshape(n, n) > (idx[:, None] * n + idx[None, :])
    sym[upper] = xi[idx][:, idx][upper]
    return sym


def test_extraction_splits_a_tie_at_rank_k_by_bin():
    n = 16
    b = W().OceanBatch(n, 1)
    b.set_params(damping=0.0, wind_dir_y=0.4142135)
    b.prepare(xi=mirrored_xi(n)[None])
    h0, _ = b.read_spectrum(0)
    p = WV.power(h0)
    idx = (n - np.arange(n)) % n
    assert np.array_equal(p[1:, 1:], p[idx][:, idx][1:, 1:])
    for k in (1, 2, 3, 7, 8, 33, 255, 4096):
        rows = check_extraction(b, 0, k, 1000.0, f"mirrored K={k}")
        if k in (1, 3, 7, 33):
            last = int(rows["bin"][-1])
            partner = ((n - last // n) % n) * n + (n - last % n) % n
            assert p.flat[partner] == p.flat[last] and partner > last and partner not in rows["bin"], k
    b.close()


def test_lifetime_and_errors():
    w = W()
    L, A = w._abi.lib(), w._abi
    n = 16
    b = w.OceanBatch(n, 2)
    cnt = C.c_uint32(7)
    assert L.ocean_extract_waves(b._h, 0, 16, None, C.byref(cnt), None) == E_NOT_READY      # before Prepare
    b.prepare(seed=1)
    for bad in (0, 4097):
        assert L.ocean_extract_waves(b._h, 0, bad, None, C.byref(cnt), None) == E_INVALID
    assert L.ocean_extract_waves(b._h, 2, 16, None, C.byref(cnt), None) == E_INVALID         # a tile outside the batch
    assert L.ocean_extract_waves(b._h, 0, 16, None, None, None) == E_INVALID
    assert L.ocean_get_waves(b._h, 0, None, C.byref(cnt)) == E_NOT_READY
    s = b._surface(0, (1.0,), n, 1.0, -1.0, 0)
    xz, out = np.zeros((1, 2), f32), np.zeros((2, 4), f32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for fn in (L.ocean_eval_waves, L.ocean_query_waves):
        assert fn(b._h, C.byref(s), 0.0, ptr(xz), 1, ptr(out[0]), ptr(out[1])) == E_NOT_READY           # no set yet
    assert L.ocean_extract_waves(b._h, 0, 16, None, C.byref(cnt), None) == 0 and cnt.value == 16        # rows and energy may be NULL
    s2 = b._surface(0, (1.0, 2.0), n, 1.0, -1.0, 0)
    for fn in (L.ocean_eval_waves, L.ocean_query_waves):
        assert fn(b._h, C.byref(s), 0.0, ptr(xz), 1, ptr(out[0]), ptr(out[1])) == 0
        assert fn(b._h, C.byref(s2), 0.0, ptr(xz), 1, ptr(out[0]), ptr(out[1])) == E_NOT_READY          # tile 1 of the surface has no set
        assert fn(b._h, C.byref(s), 0.0, None, 0, None, None) == 0                                      # points == 0: pointers not looked at
        assert fn(b._h, C.byref(s), float("nan"), ptr(xz), 1, ptr(out[0]), ptr(out[1])) == E_INVALID
        assert fn(b._h, C.byref(s), float("inf"), ptr(xz), 1, ptr(out[0]), ptr(out[1])) == E_INVALID
        assert fn(b._h, C.byref(s), 0.0, None, 1, ptr(out[0]), ptr(out[1])) == E_INVALID
    # hand-made rows: checked on the host, the old set stays after a rejected upload
    rows = b.get_waves(0)
    for field, value in (("re", np.nan), ("kx", np.inf), ("jx", n // 2), ("jz", -n // 2 - 1)):
        bad = rows.copy()
        bad[field][3] = value
        with pytest.raises(w.OceanError) as e:
            b.set_waves(bad, 0)
        assert e.value.code == E_INVALID
    assert b.get_waves(0).tobytes() == rows.tobytes()
    odd = rows.copy()
    odd["bin"], odd["reserved"] = 0xdeadbeef, np.nan                 # not looked at
    b.set_waves(odd[:5], 1)
    assert b.get_waves(1).tobytes() == odd[:5].tobytes()
    b.set_waves(rows[:0], 1)                                        # a count of 0 drops the set
    assert L.ocean_get_waves(b._h, 1, None, C.byref(cnt)) == E_NOT_READY
    b.prepare(seed=2)                                               # Prepare drops every set
    assert L.ocean_get_waves(b._h, 0, None, C.byref(cnt)) == E_NOT_READY
    b.extract_waves(8, 0)
    b.set_tile_size(32)                                             # ... and so does a new tile size
    assert L.ocean_get_waves(b._h, 0, None, C.byref(cnt)) == E_NOT_READY
    b.close()


# ---- evaluation ------------------------------------------------------------------------------------------------------------------------

N = 64
LENGTHS = tuple(1000.0 / (1.0 + 0.5 * c) for c in range(8))


@pytest.fixture(scope="module")
def gentle():
    """Eight gentle 64^2 seas with their extracted sets (K = 256): (batch, sets)."""
    b = W().OceanBatch(N, 8)
    for c, L in enumerate(LENGTHS):
        b.set_params(c, tile_length=L, **GENTLE)
    b.prepare(seed=0x5EED0001)
    sets = [b.extract_waves(256, c)[0] for c in range(8)]
    yield b, sets
    b.close()


def surface_of(sets, cascades, first=0, toffs=None, choppy=-1.0, lam=-1.0, lengths=LENGTHS, grid=N, vd=None):
    vd = lengths[first] / grid if vd is None else vd
    return WV.Surface(sets[first:first + cascades], N, [lam] * cascades, lengths[first:first + cascades], SCALES8[:cascades], grid, vd, choppy,
                      None if toffs is None else toffs[first:first + cascades])


def points(S, count, kind, seed=0):
    """Rest points: texel centres and corners of cascade 0, random ones, or far from the origin (|u s N| near 2^20)."""
    rng = np.random.default_rng(seed)
    if kind == "far":
        u = rng.uniform(0.9, 1.0, (count, 2)) * 2.0 ** 20 / S.n * rng.choice([-1.0, 1.0], (count, 2))
        return (u * S.grid * S.vd).astype(f32)
    c = WV.texel_centres(S.n, S.n, S.vd * S.grid / S.n)
    corners = (c.astype(np.float64) + 0.5 * S.vd * S.grid / S.n).astype(f32)
    rnd = rng.uniform(-3.0, 3.0, (count, 2)) * S.grid * S.vd
    pool = np.concatenate([c[rng.permutation(len(c))[:count]], corners[rng.permutation(len(c))[:count]], rnd.astype(f32)])
    return pool[rng.permutation(len(pool))[:count]].astype(f32)


def device_form(b, fn, xz, t, S, first, iterations=None):
    import torch
    d_xz = torch.from_numpy(np.ascontiguousarray(xz)).cuda()
    d_out = torch.full((2, len(xz), 4), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    kw = {} if iterations is None else dict(iterations=iterations)
    fn(d_xz.data_ptr(), len(xz), d_out[0].data_ptr(), d_out[1].data_ptr(), t, first, S.scales, S.grid, S.vd, S.choppy, **kw)
    b.synchronize()
    o = d_out.cpu().numpy()
    return o[0], o[1]


def forward(b, S, t, xz, first=0):
    """Host form, device form (the same bits), the float64 restatement and the error / bound ratio per channel."""
    pos, nrm = b.eval_waves(xz, t, first, S.scales, S.grid, S.vd, S.choppy)
    dpos, dnrm = device_form(b, b.eval_waves_device, xz, t, S, first)
    assert pos.tobytes() == dpos.tobytes() and nrm.tobytes() == dnrm.tobytes()
    rpos, rnrm, _ = WV.eval_waves(S, t, xz)
    bp, bn = WV.bound(S, float(np.abs(xz[:, 0]).max()), float(np.abs(xz[:, 1]).max()))
    assert np.all(np.isfinite(bp)) and np.all(np.isfinite(bn))
    assert np.all(nrm[:, 3] == 0.0)
    ep, en = np.abs(pos - rpos).max(axis=0), np.abs(nrm - rnrm).max(axis=0)[:3]
    return ep / bp, en / bn[:3]


RATIOS = []


def held(ratios, what):
    rp, rn = ratios
    print(f"err / bound  {what}: pos {np.array2string(rp, precision=4)}  nrm {np.array2string(rn, precision=4)}")
    RATIOS.append(max(float(rp.max()), float(rn.max())))
    assert rp.max() <= 2.0 and rn.max() <= 2.0, (what, rp, rn)


@pytest.mark.parametrize("cascades", [1, 3, 8])
def test_evaluation_within_the_bound(gentle, cascades):
    """The extracted sets of the gentle seas: 1, 3 and 8 cascades with incommensurate uv scales; 1, 255, 256, 257 and 4099 points at texel
    centres, corners and anywhere; t = 0, negative and 2.5e6 s; far from the origin; with time offsets.  Every output channel within twice
    the derived bound.  Largest error / bound ratio seen on the MI355X over all of these and the hand-made sets below: 0.68, in
    the position's x and z, where most of the bound is the rounding of x + displacement itself; 0.12 in the height, 0.31 in the normal,
    0.46 in the Jacobian slot (all at K = 1; with K = 256 the height stays below 0.01: the bound's K/8 term assumes every partial sum
    as large as the sum of all amplitudes).  `held` prints every ratio."""
    b, sets = gentle
    S = surface_of(sets, cascades)
    assert WV.steepness(S) <= 0.5, WV.steepness(S)              # sum a |k| <= 0.5: 1 + choppy S.z >= 0.5, the normal is Lipschitz in S
    for count, t in ((1, 0.0), (255, -3.7), (256, 7.3), (257, 2.5e6), (4099, 1234.5)):
        held(forward(b, S, t, points(S, count, "mixed", count)), f"{cascades} cascades, {count} points, t = {t}")
    held(forward(b, S, 7.3, points(S, 257, "far")), f"{cascades} cascades, far from the origin")
    toffs = [0.0, 11.5, -3.25, 100.0, 0.5, 7.0, -40.0, 2.0]
    b.set_time_offsets(toffs)
    try:
        held(forward(b, surface_of(sets, cascades, toffs=toffs), 7.3, points(S, 257, "mixed", 5)), f"{cascades} cascades, time offsets")
    finally:
        b.set_time_offsets(None)
    if cascades == 3:           # a tile range inside the batch
        S2 = surface_of(sets, 3, first=2)
        held(forward(b, S2, -3.7, points(S2, 257, "mixed", 9), first=2), "tiles 2 .. 4")


def test_evaluation_of_hand_made_sets(gentle):
    """A Nyquist wave (jx = -N/2), the largest |j|, a zero-amplitude row, K = 1 and K = 4096 (every bin of the lattice)."""
    b, sets = gentle
    L = LENGTHS[0]
    row = lambda jx, jz, re, im: WV.hand_row(N, L, jx, jz, re, im, float(np.sqrt(f32(9.81) * f32(2 * np.pi / L * np.hypot(jx, jz)))))
    rng = np.random.default_rng(4)
    every = np.concatenate([row(jx, jz, *(rng.uniform(-1e-4, 1e-4, 2) if (jx, jz) != (0, 0) else (0.0, 0.0)))
                            for jz in range(-N // 2, N // 2) for jx in range(-N // 2, N // 2)])
    edge = np.concatenate([row(-N // 2, 0, 0.02, -0.01), row(-N // 2, -N // 2, 0.004, 0.003), row(N // 2 - 1, N // 2 - 1, -0.003, 0.002),
                           row(5, -7, 0.0, 0.0), row(0, -N // 2, 0.01, 0.0), row(3, 2, 0.1, -0.2)])
    try:
        for name, rows in (("K = 1", row(3, -2, 0.3, 0.1)), ("edges", edge), ("K = 4096", every)):
            b.set_waves(rows, 0)
            assert b.get_waves(0).tobytes() == rows.tobytes()
            S = WV.Surface([rows], N, [-1.0], [L], [1.0], N, L / N)
            assert WV.steepness(S) <= 0.5, (name, WV.steepness(S))
            for t in (0.0, -3.7, 2.5e6):
                held(forward(b, S, t, points(S, 257, "mixed", 11)), f"hand-made {name}, t = {t}")
            held(forward(b, S, 1.0, points(S, 64, "far", 2)), f"hand-made {name}, far")
    finally:
        b.set_waves(sets[0], 0)


def frame_tolerance(S, rows, disp, nmap, amp, xmax):
    """The project's parity bound for the frame, 1e-5 * max|channel| of the maps that frame wrote (disp, nmap: the two maps read back;
    the height channel is disp.y * A), carried to the vertex stage's outputs, plus the derived bound of the proxy: (pos[4], normal).
    The sums' ceilings (sum_max) appear only where a BOUND of a sum is needed: the normal's denominators 1 + choppy S.z >= m and the
    Jacobian's other factor."""
    bp, bn = WV.bound(S, xmax, xmax)
    M = WV.sum_max(rows)
    lam, ch = abs(S.lams[0]), abs(S.choppy)
    top = lambda a: float(np.abs(a).max())
    par_d = 1e-5 * np.array([top(disp[..., 0]), top(disp[..., 1]) * amp, top(disp[..., 2])])      # disp.x / .z carry lambda already
    par_n = 1e-5 * np.array([top(nmap[..., c]) for c in range(4)])
    tol_w = bp[3] + lam * (par_n[2] * (1.0 + lam * M[6]) + par_n[3] * (1.0 + lam * M[5]))
    mx, mz = 1.0 - ch * M[5], 1.0 - ch * M[6]
    tol_n = bn[0] + par_n[0] / mx + M[3] * ch * par_n[2] / mx ** 2 + par_n[1] / mz + M[4] * ch * par_n[3] / mz ** 2
    return np.append(par_d + bp[:3], tol_w), tol_n


def against_the_frame(b, n, rows, length, lam, choppy, t, what):
    """The vertex stage on a grid of 2N quads at uv scale 1 puts its odd vertices on texel centres; the proxy at the same rest points.
    Position and normal are compared with what ocean_displace_grid wrote.  Its w is the map's D.w, which a FULL7 frame leaves at 1 (and a
    JACOBIAN frame fills with the full determinant, cross term included, which the proxy's diagonal J does not have): the proxy's
    out_pos.w is therefore compared with the diagonal Jacobian (1 + lam N.z)(1 + lam N.w) of the frame's normal map at the same texels,
    the one the foam update and the spray emitters take from a FULL7 frame."""
    vd = 0.5                                                         # a power of two: (xi * vd) / vd is xi again
    amp = float(b.compute_waves(t)[0])
    disp, nmap = (m[0].astype(np.float64) for m in b.read_maps(0, 1))
    pos, nrm = b.displace_grid(0, 2 * n, vd, 1.0, choppy)
    side = 2 * n + 1
    pos, nrm = pos.reshape(side, side, 4)[1::2, 1::2].reshape(-1, 4), nrm.reshape(side, side, 4)[1::2, 1::2].reshape(-1, 4)
    assert np.all(pos[:, 3] == 1.0)                                  # FULL7: the Jacobian slot is not filled
    want = pos.astype(np.float64)
    want[:, 3] = ((1.0 + lam * nmap[..., 2]) * (1.0 + lam * nmap[..., 3])).reshape(-1)
    xi = (np.arange(1, side, 2) - n).astype(f32) * f32(vd)
    xz = np.stack(np.meshgrid(xi, xi), axis=-1).reshape(-1, 2).astype(f32)
    got_p, got_n = b.eval_waves(xz, t, 0, (1.0,), 2 * n, vd, choppy)
    S = WV.Surface([rows], n, [lam], [length], [1.0], 2 * n, vd, choppy)
    tol_p, tol_n = frame_tolerance(S, rows, disp, nmap, amp, float(np.abs(xz).max()))
    assert np.isfinite(tol_n), what
    ep, en = np.abs(got_p - want).max(axis=0), np.abs(got_n - nrm).max(axis=0)[:3]
    print(f"proxy against the frame, {what}: pos err {ep} tol {tol_p}; nrm err {en} tol {tol_n}")
    assert np.all(ep <= tol_p) and np.all(en <= tol_n), (what, ep, tol_p, en, tol_n)


@pytest.mark.parametrize("n", [64, 256])
def test_the_proxy_is_the_frame_for_a_sparse_sea(n):
    b = W().OceanBatch(n, 1)
    b.set_params(**SPC.gpu_params())
    b.prepare(xi=SPC.sparse_xi(n))
    rows, _ = b.extract_waves(64, 0)
    assert len(rows) == len(SPC.sparse_bins(n)) - 1
    for t in (0.0, 7.3):
        against_the_frame(b, n, rows, SPC.PARAMS["length"], SPC.PARAMS["lam"], -1.0, t, f"sparse {n}, t = {t}")
    b.close()


def test_the_proxy_is_the_frame_for_a_whole_phillips_sea():
    """K = 4096 = N^2 takes every candidate of a 64^2 sea: the whole sea, not a truncation."""
    n = 64
    b = W().OceanBatch(n, 1)
    b.set_params(tile_length=1000.0, **dict(GENTLE, phillips_const=2e-10))      # (sum a |kx ux| over ALL bins stays below 0.5)
    b.prepare(seed=0x5EED0002)
    rows, energy = b.extract_waves(4096, 0)
    h0, _ = b.read_spectrum(0)
    assert len(rows) == int((WV.power(h0) > 0).sum())
    assert abs(energy / b.spectrum_moments(0)[0] - 1.0) < 1e-12          # the captured share is all of it
    for t in (0.0, -3.0):
        against_the_frame(b, n, rows, 1000.0, -1.0, -1.0, t, f"phillips 64, t = {t}")
    b.close()


def test_the_inverse(gentle):
    """ocean_query_waves against the float64 Newton restatement on the gentle sea: residual below 1e-4 m, and
    |H_gpu - H_ref| <= bound_h + G (res_gpu + res_ref) / (1 - rho); the same with one iteration; a NaN point disturbs no other row."""
    b, sets = gentle
    for cascades in (1, 3):
        S = surface_of(sets, cascades)
        G = WV.steepness(S)
        assert G <= 0.5
        xz = points(S, 257, "mixed", 21)
        bp, _ = WV.bound(S, float(np.abs(xz[:, 0]).max()), float(np.abs(xz[:, 1]).max()))
        for iterations in (8, 1):
            pos, nrm = b.query_waves(xz, 2.0, 0, S.scales, S.grid, S.vd, S.choppy, iterations)
            dpos, dnrm = device_form(b, b.query_waves_device, xz, 2.0, S, 0, iterations)
            assert pos.tobytes() == dpos.tobytes() and nrm.tobytes() == dnrm.tobytes()
            rpos, rnrm = WV.query_waves(S, 2.0, xz, iterations)
            if iterations == 8:
                assert nrm[:, 3].max() < 1e-4, nrm[:, 3].max()
            tol = bp[1] + G * (nrm[:, 3].astype(np.float64) + rnrm[:, 3]) / (1.0 - G)
            err = np.abs(pos[:, 1] - rpos[:, 1])
            print(f"inverse, {cascades} cascades, K = {iterations}: residual {nrm[:, 3].max():.3g} (ref {rnrm[:, 3].max():.3g}), "
                  f"height err / tol {float((err / tol).max()):.4f}")
            assert np.all(err <= tol), (cascades, iterations, float((err / tol).max()))
        bad = xz.copy()
        bad[100] = (np.nan, 3.0)
        p2, n2 = b.query_waves(bad, 2.0, 0, S.scales, S.grid, S.vd, S.choppy, 1)
        keep = np.arange(len(xz)) != 100
        assert p2[keep].tobytes() == pos[keep].tobytes() and n2[keep].tobytes() == nrm[keep].tobytes()


def test_cpp_host_matches_the_python_binding(tmp_path):
    """tests/cpp/waves_demo.cpp: rows, inverse and forward evaluation through the C ABI from C++, bit for bit what the binding returns."""
    import os
    import subprocess
    w = W()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "waves_demo"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"),
                    os.path.join(root, "tests", "cpp", "waves_demo.cpp"), "-o", str(exe),
                    "-L", os.path.dirname(w._abi.LIB_PATH), "-locean_hip", "-Wl,-rpath," + os.path.dirname(w._abi.LIB_PATH),
                    "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = tmp_path / "waves.bin"
    r = subprocess.run([str(exe), "64", "128", str(out), "2.0"], capture_output=True, text=True, check=True)
    n, count, share, pts = r.stdout.split()
    count, pts = int(count), int(pts)
    raw = np.fromfile(out, dtype=np.uint8)
    crows = raw[:48 * count].view(WV.WAVE_DTYPE)
    f = raw[48 * count:].view(f32)
    xz = f[:2 * pts].reshape(pts, 2)
    cq = f[2 * pts:].reshape(4, pts, 4)
    b = w.OceanBatch(64, 1)
    b.set_params(phillips_const=5e-11)
    b.prepare(seed=42)
    rows, energy = b.extract_waves(128, 0)
    assert count == 128 and rows.tobytes() == crows.tobytes()
    assert float(share) == pytest.approx(energy / b.spectrum_moments(0)[0], abs=1e-6) and 0.5 < float(share) <= 1.0
    p = b.get_params(0)
    geo = (0, (1.0,), 64, p.tile_length / f32(64), p.lambda_)
    qpos, qnrm = b.query_waves(xz, 2.0, *geo, 8)
    epos, enrm = b.eval_waves(xz, 2.0, *geo)
    for got, want in zip(cq, (qpos, qnrm, epos, enrm)):
        assert got.tobytes() == want.tobytes()
    b.close()
