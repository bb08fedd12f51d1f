"""The LOD sampler's restatement (tests/lod.py) on the CPU: the level rule against float64, the trilinear sample against the mip chain, the
grid form against oracle/consumer.py where nothing is undersampled -- and the vetting of what tests/test_lod_sampler_gpu.py runs: its
inputs reach every branch of the level rule, its undersampled grids really differ from the plain cascade call, and every expected value
is finite.  No device."""
import numpy as np
import pytest

import crafted_maps as CM
import lod as L
from oracle import consumer as O

F = np.float32


@pytest.fixture(scope="module")
def maps():
    return CM.maps()


def test_level_rule_is_floor_log2_and_t_stays_in_the_unit_interval():
    rng = np.random.default_rng(7)
    rho = np.concatenate([np.exp2(rng.uniform(0.0, 12.0, 20000)), np.linspace(1.0, 4096.0, 4097), [np.nextafter(F(1), F(2)), np.nextafter(F(4096), F(0))]]).astype(np.float32)
    rho = rho[(rho > 1) & (rho < 4096)]
    lev, t = L.level(rho, 12)
    assert np.array_equal(lev, np.floor(np.log2(rho.astype(np.float64))).astype(np.int64))
    assert t.dtype == np.float32 and np.all(t >= 0) and np.all(t < 1)
    # t is the blend that is linear in rho: rho = 2^lev * (1 + t), exactly
    assert np.array_equal(np.ldexp(F(1) + t, lev.astype(np.int32)).astype(np.float32), rho)


def test_t_is_zero_exactly_at_powers_of_two():
    p = np.exp2(np.arange(1, 12)).astype(np.float32)
    lev, t = L.level(p, 12)
    assert np.array_equal(lev, np.arange(1, 12)) and np.all(t == 0)
    lev, t = L.level(np.nextafter(p, F(np.inf)), 12)
    assert np.array_equal(lev, np.arange(1, 12)) and np.all(t > 0)
    lev, t = L.level(np.nextafter(p, F(0)), 12)
    assert np.array_equal(lev, np.arange(0, 11)) and np.all(t > 0.999)


def test_special_cases_of_the_level_rule():
    rho = np.array([0.0, -0.0, -3.0, np.nan, 1.0, 1e-30, -np.inf], np.float32)
    lev, t = L.level(rho, 4)
    assert np.all(lev == 0) and np.all(t == 0)
    rho = np.array([16.0, 17.0, 1e30, np.inf], np.float32)
    lev, t = L.level(rho, 4)
    assert np.all(lev == 4) and np.all(t == 0)
    lev, t = L.level(np.array([np.nextafter(F(16), F(0))], np.float32), 4)
    assert lev[0] == 3 and 0.999 < t[0] < 1
    # max_level clamps: 0 = no limit, beyond log2 N = log2 N
    assert [L.lmax_of(16, m) for m in (0, 1, 3, 4, 5, 99)] == [4, 1, 3, 4, 4, 4] and L.lmax_of(4096) == 12
    lev, t = L.level(np.array([1.5, 2.0, 3.0, 100.0], np.float32), L.lmax_of(16, 1))
    assert lev.tolist() == [0, 1, 1, 1] and t.tolist() == [0.5, 0.0, 0.0, 0.0]


def test_a_texel_centre_at_its_own_level_is_that_texel(maps):
    disp, _ = maps
    levels = L.levels_of(disp[2])
    assert [l.shape[0] for l in levels] == [16, 8, 4, 2, 1]
    for l, tex in enumerate(levels):
        w = tex.shape[0]
        j = (np.arange(w, dtype=np.float32) + F(0.5)) / F(w)
        us, vs = [a.ravel() for a in np.meshgrid(j, j)]
        lev, t = L.level(np.full(us.shape, 2.0 ** l, np.float32), 4)
        assert np.all(lev == l) and np.all(t == 0)
        got = L.sample_lod(levels, lev, t, us, vs)
        assert np.array_equal(got.view(np.uint32), tex.reshape(-1, 4).view(np.uint32)), l
    # half way between two levels (rho = 1.5 * 2^l) a texel centre of the UPPER level blends it with the four texels under it
    lev, t = L.level(np.array([3.0], np.float32), 4)
    got = L.sample_lod(levels, lev, t, np.array([0.375], np.float32), np.array([0.625], np.float32))
    a = O.sample_linear_repeat(levels[1], np.array([0.375], np.float32), np.array([0.625], np.float32))
    assert np.array_equal(got, a * F(0.5) + levels[2][2, 1][None] * F(0.5))


def test_zero_footprints_give_the_cascade_oracle_bit_for_bit(maps):
    disp, nrm = maps
    for grid in CM.VERTEX_GRIDS:
        for first, count in CM.VERTEX_CASCADE_SETS:
            sl = slice(first, first + count)
            sc = CM.scales(first, count, 2.5)
            want = CM.bits(*O.displace_grid_cascades(disp[sl], nrm[sl], CM.CPU_AMPS[sl], sc, grid, CM.VD, L.CHOPPY))
            # a zero vertex distance would be a zero footprint but no mesh: scale the footprint away instead
            got = CM.bits(*L.displace_grid_lod(disp[sl], nrm[sl], CM.CPU_AMPS[sl], sc, grid, CM.VD, L.CHOPPY, scale=1e-30))
            CM.assert_same_bits(got, want, f"grid {grid} tiles {first}..{first + count - 1}")
    xzf = L.point_set(257, CM.GRID, CM.VD)
    xzf[:, 2] = 0.0
    keep = L.specified_rows(xzf)
    pos, nrm_out, seen = L.sample_surface_lod(disp[:3], nrm[:3], CM.CPU_AMPS[:3], CM.scales(0, 3), CM.GRID, CM.VD, L.CHOPPY, xzf, detail=True)
    assert all(np.all(lev == 0) and np.all(t == 0) for lev, t in seen) and np.all(nrm_out[keep, 3] == 0)


def test_the_gpu_point_inputs_reach_every_branch_and_every_expected_value_is_finite(maps):
    disp, nrm = maps
    reached = {"level 0": 0, "t == 0 inside": 0, "t > 0": 0, "top clamp": 0, "nan": 0, "upper level 1x1": 0}
    for first, count, base, grid, vd, points, scale, max_level in L.point_cases():
        sl = slice(first, first + count)
        xzf = L.point_set(points, grid, vd)
        pos, out_nrm, seen = L.sample_surface_lod(disp[sl], nrm[sl], CM.CPU_AMPS[sl], CM.scales(first, count, base), grid, vd, L.CHOPPY, xzf,
                                                  scale, max_level, detail=True)
        keep = L.specified_rows(xzf)
        assert np.isfinite(pos[keep]).all() and np.isfinite(out_nrm[keep]).all(), (first, count, base, grid)
        lmax = L.lmax_of(L.N, max_level)
        rho_nan = np.isnan(xzf[:, 2])
        for lev, t in seen:
            reached["level 0"] += int(((lev == 0) & (t == 0) & keep & ~rho_nan).sum())
            reached["t == 0 inside"] += int(((lev > 0) & (lev < lmax) & (t == 0) & keep).sum())
            reached["t > 0"] += int(((t > 0) & keep).sum())
            reached["top clamp"] += int(((lev == lmax) & keep).sum())
            reached["nan"] += int((rho_nan & (lev == 0) & (t == 0)).sum())
            reached["upper level 1x1"] += int(((lev == 3) & (t > 0) & keep).sum())
        assert np.all(out_nrm[keep, 3] >= 0) and np.all(out_nrm[keep, 3] <= lmax)
    assert all(v > 0 for v in reached.values()), reached
    sets = {(c[0], c[1]) for c in L.point_cases()}
    assert {(0, 1), (0, 3), (0, 8)} <= sets and any(f == 3 for f, _ in sets)
    assert {c[5] for c in L.point_cases()} == set(L.POINT_COUNTS) and {(c[6], c[7]) for c in L.point_cases()} == set(L.LOD_SETTINGS)


def test_the_gpu_grid_inputs_are_what_their_lists_say(maps):
    disp, nrm = maps
    reached = {"level 0": 0, "t == 0 inside": 0, "t > 0": 0, "top clamp": 0}
    assert {g[0] for g in L.GRID_PLAIN + L.GRID_UNDER} == set(CM.VERTEX_GRIDS)
    for plain, cases in ((True, L.GRID_PLAIN), (False, L.GRID_UNDER)):
        for grid, first, count, base, scale, max_level in cases:
            sl = slice(first, first + count)
            sc = CM.scales(first, count, base)
            texels = [s * L.N / grid for s in sc]
            assert (max(texels) <= 1.0) == plain, (grid, first, count, base)
            got_pos, got_nrm, seen = L.displace_grid_lod(disp[sl], nrm[sl], CM.CPU_AMPS[sl], sc, grid, CM.VD, L.CHOPPY, scale, max_level, detail=True)
            got = CM.bits(got_pos, got_nrm)
            assert np.isfinite(got_pos).all() and np.isfinite(got_nrm).all() and np.all(got_nrm[:, 3] == 0)
            flat = CM.bits(*O.displace_grid_cascades(disp[sl], nrm[sl], CM.CPU_AMPS[sl], sc, grid, CM.VD, L.CHOPPY))
            differ = (got != flat).any(axis=1)
            if plain:
                assert all(np.all(lev == 0) and np.all(t == 0) for lev, t in seen) and not differ.any(), (grid, first, count, base)
            else:
                assert differ.sum() > len(differ) / 2, (grid, first, count, base, int(differ.sum()), len(differ))
            lmax = L.lmax_of(L.N, max_level)
            for lev, t in seen:
                reached["level 0"] += int(lev[0] == 0 and t[0] == 0)
                reached["t == 0 inside"] += int(0 < lev[0] < lmax and t[0] == 0)
                reached["t > 0"] += int(t[0] > 0)
                reached["top clamp"] += int(lev[0] == lmax)
    assert all(v > 0 for v in reached.values()), reached


# ---- the inputs of tests/test_chain_readers_sizes_gpu.py: tiles of 256^2 ---------------------------------------------------------------------
def test_the_generators_give_the_16_squared_inputs_unchanged_at_their_defaults():
    """The n parameter's default is the crafted maps' size: the point set of tests/test_lod_sampler_gpu.py is, byte for byte, what the
    generator gave before it took an n (the digest is of that array), and spelling the default out changes nothing."""
    import hashlib
    xzf = L.point_set(1000, CM.GRID, CM.VD)
    assert hashlib.sha256(xzf.tobytes()).hexdigest() == "d8c03c9c99f94d0839cc45ef4db7279f6d353788aa7f28da326490d8f2bebd75"
    assert np.array_equal(L.point_set(1000, CM.GRID, CM.VD, n=16).view(np.uint32), xzf.view(np.uint32))
    assert L.footprint_texels() is L.FOOTPRINT_TEXELS and L.point_meshes() == L.POINT_MESHES
    assert L.point_cases() == L.point_cases(L.CASCADE_SETS, L.POINT_COUNTS, L.LOD_SETTINGS, L.POINT_MESHES) and len(L.point_cases()) == 36


def test_the_256_footprints_are_what_the_list_says():
    f = L.footprint_texels(256)
    powers = [2.0 ** k for k in range(0, 9)]
    assert set(powers) <= set(f) and all(any(a < x < b for x in f) for a, b in zip(powers, powers[1:]))
    assert {0.0, -1.0, 0.5, 1.0e-30, np.inf} <= set(f) and any(256 < x < np.inf for x in f) and any(0 < x < 1 for x in f)
    xzf = L.point_set(257, CM.GRID, CM.VD, n=256)
    assert np.isnan(xzf[L.NAN_ROW, 2]) and np.isinf(xzf[L.INF_ROW, 0]) and (~L.specified_rows(xzf)).sum() == 1
    # every footprint of the table is reached by a count that is at least its length
    want = np.array(f, np.float64) * (CM.GRID * CM.VD / 256)
    assert {float(x) for x in xzf[np.isfinite(xzf[:, 2]), 2]} == {float(np.float32(x)) for x in want if np.isfinite(x)}


@pytest.fixture(scope="module")
def maps256():
    return L.random_maps(L.SIZES_N, L.SIZES_TILES, 20262)


def test_the_256_point_inputs_reach_every_level_and_every_expected_value_is_finite(maps256):
    """Every level 0 .. 8 occurs as lev with t == 0, every level 0 .. 7 with t != 0 (on the last level t is 0 by the rule), beside the
    branches the 16^2 inputs are vetted for."""
    disp, nrm = maps256
    n, top = L.SIZES_N, 8
    flat, blend = np.zeros(top + 1, np.int64), np.zeros(top + 1, np.int64)
    reached = {"t == 0 inside": 0, "top clamp": 0, "max_level clamp": 0, "nan": 0, "upper level 1x1": 0}
    cases = L.sizes_point_cases()
    for first, count, base, grid, vd, points, scale, max_level in cases:
        sl = slice(first, first + count)
        xzf = L.point_set(points, grid, vd, n=n)
        pos, out_nrm, seen = L.sample_surface_lod(disp[sl], nrm[sl], CM.CPU_AMPS[sl], CM.scales(first, count, base), grid, vd, L.CHOPPY, xzf,
                                                  scale, max_level, detail=True)
        keep = L.specified_rows(xzf)
        assert np.isfinite(pos[keep]).all() and np.isfinite(out_nrm[keep]).all(), (first, count, base, grid)
        lmax = L.lmax_of(n, max_level)
        rho_nan = np.isnan(xzf[:, 2])
        for lev, t in seen:
            ok = keep & ~rho_nan
            flat += np.bincount(lev[ok & (t == 0)], minlength=top + 1)
            blend += np.bincount(lev[ok & (t != 0)], minlength=top + 1)
            reached["t == 0 inside"] += int(((lev > 0) & (lev < lmax) & (t == 0) & keep).sum())
            reached["top clamp"] += int(((lev == top) & keep).sum())
            reached["max_level clamp"] += int(((lev == lmax) & (lmax < top) & keep).sum())
            reached["nan"] += int((rho_nan & (lev == 0) & (t == 0)).sum())
            reached["upper level 1x1"] += int(((lev == top - 1) & (t > 0) & keep).sum())
            assert np.all(lev <= lmax) and np.all(t >= 0) and np.all(t < 1)
        assert np.all(out_nrm[keep, 3] >= 0) and np.all(out_nrm[keep, 3] <= lmax)
    assert np.all(flat > 0) and np.all(blend[:top] > 0) and blend[top] == 0, (flat, blend)
    assert all(v > 0 for v in reached.values()), reached
    assert {(c[0], c[1]) for c in cases} == set(L.SIZES_CASCADE_SETS) and {c[2] for c in cases} == set(L.UV_BASES)
    assert {(c[5], c[6], c[7]) for c in cases} == {(p, s, m) for p in L.SIZES_POINT_COUNTS for s, m in L.SIZES_LOD_SETTINGS}
    assert all(first + count <= L.SIZES_TILES for first, count in L.SIZES_CASCADE_SETS)


def test_the_256_grid_inputs_are_what_their_lists_say(maps256):
    disp, nrm = maps256
    n, top = L.SIZES_N, 8
    lone, mixed = set(), 0
    for plain, cases in ((True, L.SIZES_GRID_PLAIN), (False, L.SIZES_GRID_UNDER)):
        for grid, first, count, base, scale, max_level in cases:
            sl = slice(first, first + count)
            sc = CM.scales(first, count, base)
            assert (max(scale * s * n / grid for s in sc) <= 1.0) == plain, (grid, first, count, base)
            got_pos, got_nrm, seen = L.displace_grid_lod(disp[sl], nrm[sl], CM.CPU_AMPS[sl], sc, grid, CM.VD, L.CHOPPY, scale, max_level, detail=True)
            got = CM.bits(got_pos, got_nrm)
            assert np.isfinite(got_pos).all() and np.isfinite(got_nrm).all() and np.all(got_nrm[:, 3] == 0)
            flat = CM.bits(*O.displace_grid_cascades(disp[sl], nrm[sl], CM.CPU_AMPS[sl], sc, grid, CM.VD, L.CHOPPY))
            differ = (got != flat).any(axis=1)
            if plain:
                assert all(np.all(lev == 0) and np.all(t == 0) for lev, t in seen) and not differ.any(), (grid, first, count, base)
            else:
                assert differ.sum() > len(differ) / 2, (grid, first, count, base, int(differ.sum()), len(differ))
            levels = [(int(lev[0]), float(t[0])) for lev, t in seen]
            assert all(np.all(lev == lev[0]) and np.all(t == t[0]) for lev, t in seen)          # one footprint: one level per cascade
            assert all(l <= L.lmax_of(n, max_level) for l, _ in levels)
            if count == 1:
                lone.add(levels[0])
            mixed += int(len({l for l, _ in levels}) > 1 and any(t > 0 for _, t in levels))
    assert {(3, 0.0), (6, 0.0), (top, 0.0)} <= lone and any(l == 0 and t > 0 for l, t in lone), lone
    assert mixed >= 2
