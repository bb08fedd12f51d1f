"""numpy restatement of the LOD sampler (include/ocean_consumers.h: ocean_sample_surface_lod, ocean_displace_grid_lod): the level rule, the
trilinear sample, the point form and the grid form, in the fp32 order the header states -- and the inputs the GPU tests run, which
tests/test_lod.py vets on the CPU: at their defaults the ones for the crafted 16^2 maps (tests/test_lod_sampler_gpu.py), with n = 256 the
ones for a real sea of 256^2 tiles (tests/test_chain_readers_sizes_gpu.py).  The restatement itself is general in the tile size.  TEST
INFRASTRUCTURE ONLY (tests/test_lod.py, tests/test_bounds.py, tests/test_lod_sampler_gpu.py, tests/test_chain_readers_sizes_gpu.py).  The
bilinear sample and the mip chain are oracle/consumer.py's, imported and not copied."""
import numpy as np

import crafted_maps as CM
from oracle.consumer import mip_chain, sample_linear_repeat

F = np.float32


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def lmax_of(n, max_level=0):
    top = int(n).bit_length() - 1
    return min(top, int(max_level)) if max_level else top


def level(rho, lmax):
    """(lev int64, t float32) of the ratios rho (float32): level 0 unless rho > 1 (0, negative, NaN), the last level from 2^lmax on
    (+inf), in between rho's exponent and rho / 2^lev - 1 -- np.frexp gives rho = m * 2^e with m in [0.5, 1), so lev = e - 1, t = 2m - 1."""
    rho = np.asarray(rho, dtype=np.float32)
    lev = np.zeros(rho.shape, np.int64)
    t = np.zeros(rho.shape, np.float32)
    with np.errstate(invalid="ignore"):
        hi = rho >= F(2.0 ** lmax)
        mid = (rho > F(1.0)) & ~hi
    m, e = np.frexp(rho[mid])
    lev[mid] = e - 1
    t[mid] = m * F(2.0) - F(1.0)
    lev[hi] = lmax
    return lev, t


def levels_of(tex):
    """Level 0 (the map) and the levels of oracle.consumer.mip_chain behind it."""
    return [np.ascontiguousarray(tex, dtype=np.float32)] + mip_chain(tex)


def sample_lod(levels, lev, t, us, vs):
    """A = the bilinear sample of level lev; where t != 0, B = that of level lev + 1 and A * (1 - t) + B * t per channel."""
    out = np.zeros(us.shape + (4,), np.float32)
    for l in np.unique(lev):
        at = lev == l
        a = sample_linear_repeat(levels[l], us[at], vs[at])
        tt = t[at]
        blend = tt != F(0.0)
        if blend.any():
            b = sample_linear_repeat(levels[l + 1], us[at][blend], vs[at][blend])
            tb = tt[blend][:, None]
            a[blend] = a[blend] * (F(1.0) - tb) + b * tb
        out[at] = a
    return out


def texels_per_metre(uv_scale, n, grid, vertex_distance):
    return np.abs((F(uv_scale) * F(n)) / (F(grid) * F(vertex_distance)))


def _combine(disps, nrms, amps, uv_scales, grid, vertex_distance, choppy, px, pz, u, v, f, scale, max_level, detail):
    n = disps[0].shape[0]
    lmax = lmax_of(n, max_level)
    fs = f * F(scale)
    dx = np.zeros(u.shape, np.float32); dy = dx.copy(); dz = dx.copy()
    s = np.zeros(u.shape + (4,), np.float32)
    w = np.full(u.shape, np.finfo(np.float32).max, np.float32)
    lam = np.zeros(u.shape, np.float32)
    seen = []
    for d, q, amp, sc in zip(disps, nrms, amps, uv_scales):
        us, vs = u * F(sc), v * F(sc)
        lev, t = level(fs * texels_per_metre(sc, n, grid, vertex_distance), lmax)
        sd = sample_lod(levels_of(d), lev, t, us, vs)
        dx = dx + sd[:, 0]; dy = dy + sd[:, 1] * F(amp); dz = dz + sd[:, 2]
        w = np.minimum(w, sd[:, 3])
        s = s + sample_lod(levels_of(q), lev, t, us, vs)
        lam = np.maximum(lam, lev.astype(np.float32) + t)
        seen.append((lev, t))
    pos = np.stack([px + dx, F(0.0) + dy, pz + dz, w], axis=1).astype(np.float32)
    nx = -(s[:, 0] / (F(1.0) + F(choppy) * s[:, 2]))
    nz = -(s[:, 1] / (F(1.0) + F(choppy) * s[:, 3]))
    ln = np.sqrt(nx * nx + F(1.0) + nz * nz)
    return pos, nx / ln, F(1.0) / ln, nz / ln, lam, seen


def sample_surface_lod(disps, nrms, amps, uv_scales, grid, vertex_distance, choppy, xzf, scale=1.0, max_level=0, detail=False):
    """The point form: (out_pos, out_nrm) [points, 4] float32 for xzf [points, 3]; detail=True adds [(lev, t)] per cascade."""
    xzf = np.ascontiguousarray(xzf, dtype=np.float32).reshape(-1, 3)
    x, z, f = xzf[:, 0], xzf[:, 1], xzf[:, 2]
    half = F(grid // 2)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (x / F(vertex_distance) + half) / F(grid)
        v = (z / F(vertex_distance) + half) / F(grid)
        pos, n0, n1, n2, lam, seen = _combine(disps, nrms, amps, uv_scales, grid, vertex_distance, choppy, x, z, u, v, f, scale, max_level, detail)
    nrm = np.stack([n0, n1, n2, lam], axis=1).astype(np.float32)
    return (pos, nrm, seen) if detail else (pos, nrm)


def displace_grid_lod(disps, nrms, amps, uv_scales, grid, vertex_distance, choppy, scale=1.0, max_level=0, detail=False):
    """The grid form: oracle.consumer.displace_grid_cascades' vertices and (u, v), footprint |vertex_distance| everywhere, normals.w = 0."""
    side, half = grid + 1, grid // 2
    i = np.arange(side * side)
    xi, yi = i % side - half, i // side - half
    px = xi.astype(np.float32) * F(vertex_distance)
    pz = yi.astype(np.float32) * F(vertex_distance)
    u = (xi + half).astype(np.float32) / F(grid)
    v = (yi + half).astype(np.float32) / F(grid)
    f = np.full(side * side, np.abs(F(vertex_distance)), np.float32)
    pos, n0, n1, n2, _, seen = _combine(disps, nrms, amps, uv_scales, grid, vertex_distance, choppy, px, pz, u, v, f, scale, max_level, detail)
    nrm = np.stack([n0, n1, n2, np.zeros_like(n0)], axis=1).astype(np.float32)
    return (pos, nrm, seen) if detail else (pos, nrm)


# ---- what the GPU tests run (tests/test_lod_sampler_gpu.py), vetted by tests/test_lod.py -------------------------------------------------------
N = CM.N
CHOPPY = CM.VERTEX_CHOPPY
CASCADE_SETS = ((0, 1), (0, 3), (0, 8), (3, 1), (3, 3), (3, 5))     # (first_tile, cascades): 1, 3 and 8 from tile 0; 1, 3 and to the end from tile 3
UV_BASES = (1.0, 0.37, 2.5)
POINT_COUNTS = (1, 255, 256, 257, 1000)
LOD_SETTINGS = ((1.0, 0), (1.0, 1), (1.0, 4), (0.75, 0))            # (scale, max_level): no limit, one level, log2 N spelled out; a scaled footprint
# Two meshes: the reference mesh of crafted_maps (62.5 m per texel of tile 0 at uv_scale 1), and one of a texel per metre, where
# texels_per_metre is exactly uv_scale and the footprint IS rho for tile 0 at scale 1 (powers of two give t == 0 inside the chain).
POINT_MESHES = ((CM.GRID, CM.VD), (16, 1.0))
# footprints in texels of tile 0 at uv_scale 1: both sides of 1, powers of two inside the chain, between them, the top (16) and beyond
FOOTPRINT_TEXELS = (0.0, -1.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 5.5, 8.0, 11.0, 16.0, 20.0, 1.0e6, np.inf, 0.3, 2.5, 7.0, 2.0 / 0.75, 1.0e-30)
NAN_ROW, INF_ROW = 5, 11            # in every point set with that many rows: a NaN footprint; a position that is not finite (row unspecified)
POINT_SEED = 20250


def footprint_texels(n=N):
    """Footprints in texels of tile 0 at uv_scale 1 for tiles of n^2: 0, negative, both sides of 1, every power of two up to n with one
    value between each pair, n itself, above n, far above, +inf, a few that are no power of two, and 1e-30.  n = 16: FOOTPRINT_TEXELS."""
    if n == N:
        return FOOTPRINT_TEXELS
    out = [0.0, -1.0, 0.5, 1.0]
    for k in range(int(n).bit_length() - 1):
        out += [(1.5 if k % 2 == 0 else 1.375) * 2.0 ** k, 2.0 ** (k + 1)]       # between 2^k and 2^(k+1), then 2^(k+1); the last is n
    return tuple(out + [1.25 * n, 1.0e6, np.inf, 0.3, 2.5, 7.0, 2.0 / 0.75, 1.0e-30])


def point_meshes(n=N):
    """POINT_MESHES for tiles of n^2: the reference mesh, and n quads of one metre, where texels_per_metre is exactly uv_scale."""
    return ((CM.GRID, CM.VD), (n, 1.0))


def point_set(count, grid, vertex_distance, seed=POINT_SEED, n=N):
    """xzf [count, 3]: uniform rest points over 1.4 mesh widths, footprints cycling through footprint_texels(n) (in a stride coprime to
    their number, so that every one is reached)."""
    rng = np.random.default_rng(seed + count)
    width = grid * vertex_distance
    table = footprint_texels(n)
    stride = next(s for s in (7, 11, 13) if len(table) % s)
    xzf = np.empty((count, 3), np.float32)
    xzf[:, :2] = rng.uniform(-0.7 * width, 0.7 * width, (count, 2))
    xzf[:, 2] = (np.array(table, np.float64) * (width / n))[(np.arange(count) * stride) % len(table)]
    if count > NAN_ROW:
        xzf[NAN_ROW, 2] = np.nan
    if count > INF_ROW:
        xzf[INF_ROW, 0] = np.inf
    return xzf


def specified_rows(xzf):
    """The rows whose result the contract specifies: every one with a finite position (a NaN footprint is level 0, not an error)."""
    return np.isfinite(xzf[:, 0]) & np.isfinite(xzf[:, 1])


def point_cases(cascade_sets=CASCADE_SETS, counts=POINT_COUNTS, settings=LOD_SETTINGS, meshes=POINT_MESHES):
    """(first_tile, cascades, uv_base, grid, vertex_distance, points, scale, max_level): every cascade set, uv base, mesh, count and LOD
    setting appears, in a rotation and not the full product."""
    out, k = [], 0
    for first, count in cascade_sets:
        for base in UV_BASES:
            for grid, vd in meshes:
                points = counts[k % len(counts)]
                scale, max_level = settings[k % len(settings)]
                out.append((first, count, base, grid, vd, points, scale, max_level))
                k += 1
    return out


# Grids of CM.VERTEX_GRIDS at CM.VD.  PLAIN: uv_scale * 16 / grid <= 1 for every cascade, so the LOD call is the cascade call in every bit
# (grid 16 at uv_scale 1 sits exactly on 1).  UNDER: at least one cascade undersampled, the LOD call differs on most vertices.
#   (grid, first_tile, cascades, uv_base, scale, max_level)
GRID_PLAIN = ((255, 0, 3, 1.0, 1.0, 0), (255, 0, 3, 2.5, 1.0, 0), (255, 3, 3, 0.37, 1.0, 0), (17, 0, 1, 1.0, 1.0, 0), (17, 3, 1, 0.37, 1.0, 0),
              (16, 0, 1, 1.0, 1.0, 0), (255, 0, 8, 0.37, 1.0, 1), (15, 3, 3, 0.37, 0.75, 0))
GRID_UNDER = ((16, 0, 3, 1.0, 1.0, 0), (15, 0, 8, 2.5, 1.0, 0), (3, 3, 3, 2.5, 1.0, 0), (2, 0, 8, 1.0, 1.0, 0), (1, 0, 3, 1.0, 1.0, 0),
              (255, 0, 8, 2.5, 1.0, 0), (17, 3, 3, 1.0, 1.0, 0), (17, 0, 8, 1.0, 1.0, 1), (16, 0, 3, 2.5, 0.75, 0), (16, 3, 1, 2.0, 1.0, 4))


# ---- what tests/test_chain_readers_sizes_gpu.py runs on a real sea of 256^2 tiles (six of them: crafted_maps.LENGTHS[:6]) -------------------
# A chain of 256^2 has eight levels, the last two written by the builders' second launch; level offsets, `top`, max_level and the exponent
# of rho all pass the values a 16^2 chain stops at.
SIZES_N, SIZES_TILES = 256, 6
SIZES_CASCADE_SETS = ((0, 1), (0, 3), (2, 3), (1, 5))
SIZES_POINT_COUNTS = (1, 257, 1000)
SIZES_LOD_SETTINGS = ((1.0, 0), (1.0, 1), (1.0, 5), (1.0, 8), (0.75, 0))      # no limit, one level, inside the chain, log2 N spelled out; scaled


def sizes_point_cases():
    """point_cases() for the 256^2 sea: 24 cases, every pair of (count, LOD setting) among them."""
    return point_cases(SIZES_CASCADE_SETS, SIZES_POINT_COUNTS, SIZES_LOD_SETTINGS, point_meshes(SIZES_N))


# Grids at CM.VD over the 256^2 sea, (grid, first_tile, cascades, uv_base, scale, max_level).  A cascade of uv_scale s on a grid of g quads
# has rho = scale * s * 256 / g.  PLAIN: rho <= 1 for every cascade (256 quads at uv_scale 1 sit exactly on 1).  UNDER: 255 quads blend
# level 0 with a little of level 1; 32, 4 and 1 quads at uv_scale 1 sit on levels 3, 6 and the top with t == 0; the sets of several
# cascades put them on different levels, with blends, one of them cut at max_level 5.
SIZES_GRID_PLAIN = ((256, 0, 1, 1.0, 1.0, 0), (257, 0, 3, 0.37, 1.0, 0), (300, 2, 3, 0.37, 1.0, 0), (32, 0, 3, 1.0, 1.0e-30, 0))
SIZES_GRID_UNDER = ((255, 0, 1, 1.0, 1.0, 0), (32, 0, 1, 1.0, 1.0, 0), (4, 0, 1, 1.0, 1.0, 0), (1, 0, 1, 1.0, 1.0, 0),
                    (32, 0, 3, 1.0, 1.0, 0), (5, 1, 5, 2.5, 1.0, 0), (4, 2, 3, 1.0, 1.0, 5), (3, 0, 3, 1.0, 0.75, 0))


def random_maps(n, tiles, seed):
    """(disp, nrm), each [tiles, n, n, 4] float32, of the CPU tests at sizes beyond crafted_maps: crafted_maps.maps() without its blocks."""
    rng = np.random.default_rng(seed)
    disp = rng.standard_normal((tiles, n, n, 4)) * np.array([0.5, 1.0, 0.5, 0.0])
    disp[..., 3] = rng.uniform(-1.0, 2.0, (tiles, n, n))
    nrm = np.empty((tiles, n, n, 4))
    nrm[..., :2] = 0.3 * rng.standard_normal((tiles, n, n, 2))
    nrm[..., 2:] = 0.02 * rng.standard_normal((tiles, n, n, 2))
    return disp.astype(np.float32), nrm.astype(np.float32)
