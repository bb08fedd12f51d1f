"""numpy restatement of the surface bounds (include/ocean_consumers.h: ocean_build_bounds_tiles, ocean_patch_bounds): the min/max pyramid
of a displacement map and the patch query, in the fp32 order the header states -- and the inputs the GPU tests run, which
tests/test_bounds.py vets on the CPU: at their defaults the ones for the crafted 16^2 maps (tests/test_patch_bounds_gpu.py), with n = 256
the ones for a real sea of 256^2 tiles (tests/test_chain_readers_sizes_gpu.py).  The restatement itself is general in the tile size.  TEST
INFRASTRUCTURE ONLY (tests/test_bounds.py, tests/test_bounds_tiles_gpu.py, tests/test_patch_bounds_gpu.py,
tests/test_chain_readers_sizes_gpu.py)."""
import numpy as np

import crafted_maps as CM

F = np.float32
FLT_MAX = np.finfo(np.float32).max


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def pyramid(disp):
    """[(lo, hi)] for the levels l = 1 .. log2 N of a map [N, N, 4]: node (y, x) of level l is the minimum / maximum per channel of the
    map's rows y * 2^l .. (y + 1) * 2^l - 1 and columns x * 2^l .. (x + 1) * 2^l - 1.  (min and max are exact: taken level by level here.)"""
    lo = hi = np.ascontiguousarray(disp, dtype=np.float32)
    out = []
    while lo.shape[0] > 1:
        lo = np.minimum(np.minimum(lo[0::2, 0::2], lo[0::2, 1::2]), np.minimum(lo[1::2, 0::2], lo[1::2, 1::2]))
        hi = np.maximum(np.maximum(hi[0::2, 0::2], hi[0::2, 1::2]), np.maximum(hi[1::2, 0::2], hi[1::2, 1::2]))
        out.append((lo, hi))
    return out


def _to_int(v):
    """(int)floorf(v) as the device converts: saturating, NaN -> 0 (only rows outside the supported range get there)."""
    f = np.floor(v).astype(np.float64)
    f = np.where(np.isnan(f), 0.0, f)
    return np.clip(f, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def axis_range(p0, p1, vd, grid, sc, n, pad):
    """(i0, i1) int64 of one axis with ends p0, p1 for a cascade of scale sc: t(p) as ocean_query_surface forms u and its sampler s."""
    half = F(grid // 2)
    with np.errstate(invalid="ignore", over="ignore"):
        t0 = ((p0 / F(vd) + half) / F(grid)) * F(sc) * F(n) - F(0.5)
        t1 = ((p1 / F(vd) + half) / F(grid)) * F(sc) * F(n) - F(0.5)
        return _to_int(np.fmin(t0, t1)) - pad, _to_int(np.fmax(t0, t1)) + 1 + pad


def classify(lo, hi, planes, detail=False):
    """cls per row: 0 outside (the first plane whose far corner is outside stops the walk), 1 straddles, 2 inside; 1 without planes."""
    count = lo.shape[0]
    planes = np.zeros((0, 4), np.float32) if planes is None else np.asarray(planes, dtype=np.float32).reshape(-1, 4)
    stop = np.full(count, -1, np.int64)
    if len(planes) == 0:
        cls = np.ones(count, np.float32)
        return (cls, stop) if detail else cls
    cls = np.full(count, 2.0, np.float32)
    live = np.ones(count, bool)
    for k, (a, b, c, d) in enumerate(planes):
        fx, fy, fz = (hi if a >= 0 else lo)[:, 0], (hi if b >= 0 else lo)[:, 1], (hi if c >= 0 else lo)[:, 2]
        nx, ny, nz = (lo if a >= 0 else hi)[:, 0], (lo if b >= 0 else hi)[:, 1], (lo if c >= 0 else hi)[:, 2]
        with np.errstate(invalid="ignore", over="ignore"):
            far = ((a * fx + b * fy) + c * fz) + d
            near = ((a * nx + b * ny) + c * nz) + d
            out = live & (far < 0)
            cls[out] = 0.0
            stop[out] = k
            live &= ~out
            cls[live & (near < 0)] = 1.0
    return (cls, stop) if detail else cls


def patch_bounds(disps, amps, uv_scales, grid, vd, rects, first_level=1, pad=0, planes=None, detail=False):
    """(out_lo, out_hi) [count, 4] float32 for rects [count, 4] = (x0, z0, x1, z1).  detail=True adds, per cascade, a dict of the chosen
    level, the node indices (nx0, nx1, nz0, nz1), the index ranges and whether the whole-tile node was forced (w >= N or not finite), and
    the plane at which the classification stopped (-1: it did not)."""
    rects = np.ascontiguousarray(rects, dtype=np.float32).reshape(-1, 4)
    x0, z0, x1, z1 = rects.T
    count = len(rects)
    n = disps[0].shape[0]
    top = int(n).bit_length() - 1
    first_level = max(1, int(first_level))
    finite = np.isfinite(rects).all(axis=1)
    L = np.zeros((count, 3), np.float32)
    H = np.zeros((count, 3), np.float32)
    lw = np.full(count, FLT_MAX, np.float32)
    seen = []
    for d, amp, sc in zip(disps, amps, uv_scales):
        pyr = pyramid(d)
        i0x, i1x = axis_range(x0, x1, vd, grid, sc, n, pad)
        i0z, i1z = axis_range(z0, z1, vd, grid, sc, n, pad)
        w = np.maximum(i1x - i0x, i1z - i0z) + 1
        whole = (w >= n) | ~finite
        lev = np.ones(count, np.int64)
        for k in range(1, top):
            lev += w > (1 << k)
        lev = np.maximum(lev, first_level)
        lev[whole] = top
        m = (n >> lev) - 1
        nx0, nx1, nz0, nz1 = (i0x >> lev) & m, (i1x >> lev) & m, (i0z >> lev) & m, (i1z >> lev) & m
        lo_c = np.empty((count, 4), np.float32)
        hi_c = np.empty((count, 4), np.float32)
        for l in np.unique(lev):
            at = lev == l
            lo_l, hi_l = pyr[l - 1]
            a, b, c, e = nx0[at], nx1[at], nz0[at], nz1[at]
            lo_c[at] = np.minimum(np.minimum(lo_l[c, a], lo_l[c, b]), np.minimum(lo_l[e, a], lo_l[e, b]))
            hi_c[at] = np.maximum(np.maximum(hi_l[c, a], hi_l[c, b]), np.maximum(hi_l[e, a], hi_l[e, b]))
        L[:, 0] = L[:, 0] + lo_c[:, 0]; L[:, 1] = L[:, 1] + lo_c[:, 1] * F(amp); L[:, 2] = L[:, 2] + lo_c[:, 2]
        H[:, 0] = H[:, 0] + hi_c[:, 0]; H[:, 1] = H[:, 1] + hi_c[:, 1] * F(amp); H[:, 2] = H[:, 2] + hi_c[:, 2]
        lw = np.minimum(lw, lo_c[:, 3])
        seen.append(dict(level=lev, nx0=nx0, nx1=nx1, nz0=nz0, nz1=nz1, i0x=i0x, i1x=i1x, i0z=i0z, i1z=i1z, w=w, whole=whole))
    with np.errstate(invalid="ignore", over="ignore"):
        lo = np.stack([np.fmin(x0, x1) + L[:, 0], F(0.0) + L[:, 1], np.fmin(z0, z1) + L[:, 2], lw], axis=1).astype(np.float32)
        hi = np.stack([np.fmax(x0, x1) + H[:, 0], F(0.0) + H[:, 1], np.fmax(z0, z1) + H[:, 2], np.ones(count, np.float32)], axis=1).astype(np.float32)
    hi[:, 3], stop = classify(lo, hi, planes, detail=True)
    return (lo, hi, seen, stop) if detail else (lo, hi)


def slack(disps, amps):
    """e per output channel (x, y, z, w): what the rounding of the bilinear blend can add to the largest texel a sample reads.  1 - a is
    inexact by at most 2^-25 where a < 0.5 and five rounded operations follow, each within 2^-24 relative, so a sample exceeds the largest
    texel it reads by less than 2^-21 * max|texel|; the cascade sums add nothing, because rounding is monotone (tests/test_bounds.py)."""
    e = np.zeros(4, np.float64)
    for d, amp in zip(disps, amps):
        big = np.abs(np.asarray(d, dtype=np.float64)).reshape(-1, 4).max(axis=0)
        e += 2.0 ** -21 * big * np.array([1.0, float(amp), 1.0, 0.0])
        e[3] = max(e[3], 2.0 ** -21 * big[3])
    return e


# ---- what the GPU tests run (tests/test_patch_bounds_gpu.py), vetted by tests/test_bounds.py ---------------------------------------------------
N = CM.N
RECTS = 4099                        # a count that fills neither the last wave nor the last block
RECT_SEED = 20260
NAN_ROW = 77
PADS = (0, 1, 4)
FIRST_LEVELS = (1, 3)


NODE_SEED = 20261
NODES_PER_LEVEL = 64                # of the levels below log2 n - 3, which have more nodes than that


def node_rects(grid=CM.GRID, vd=CM.VD, n=N):
    """Rectangles whose index range on a cascade of uv_scale 1 is exactly ONE node of level l = 1 .. log2 n: for every node of the levels
    from log2 n - 3 on (at most 8 x 8 nodes), and for NODES_PER_LEVEL seeded nodes of each level below (n = 16: every node of every level).
    t(p0) = k 2^l + 0.25 and t(p1) = (k + 1) 2^l - 1.75 give i0 = k 2^l, i1 = (k + 1) 2^l - 1.  On the reference mesh every end is exact.
    Returns (rects [*, 4], level [*], node y [*], node x [*])."""
    out, lv, ny, nx = [], [], [], []
    top = int(n).bit_length() - 1
    rng = np.random.default_rng(NODE_SEED + n)
    p = lambda t: ((t + 0.5) / n * grid - grid // 2) * vd
    for l in range(1, top + 1):
        ext = n >> l
        nodes = np.arange(ext * ext) if l >= top - 3 else np.sort(rng.choice(ext * ext, NODES_PER_LEVEL, replace=False))
        for y, x in zip((nodes // ext).tolist(), (nodes % ext).tolist()):
            out.append((p(x * 2 ** l + 0.25), p(y * 2 ** l + 0.25), p((x + 1) * 2 ** l - 1.75), p((y + 1) * 2 ** l - 1.75)))
            lv.append(l); ny.append(y); nx.append(x)
    return np.array(out, np.float64).astype(np.float32), np.array(lv), np.array(ny), np.array(nx)


def rect_set(grid, vd, count=RECTS, seed=RECT_SEED, n=N):
    """rects [count, 4] over a mesh of width W = grid * vd: random ones of every size from a tenth of a texel of tile 0 (n^2 texels) to
    more than the tile, ones aligned to nodes, points (x0 == x1, and z0 == z1), reversed ends, ones spanning more than a tile, and copies
    shifted by whole mesh periods to negative coordinates."""
    rng = np.random.default_rng(seed)
    w = abs(grid * vd)
    r = np.empty((count, 4), np.float64)
    centre = rng.uniform(-0.7 * w, 0.7 * w, (count, 2))
    size = w / n * np.exp2(rng.uniform(-3.3, int(n).bit_length() - 1 + 0.3, (count, 2)))    # 0.1 texel .. 1.2 tiles
    r[:, 0:2] = centre - 0.5 * size
    r[:, 2:4] = centre + 0.5 * size
    k = np.arange(count)
    big = k % 11 == 3                                                           # spanning more than a tile: 1.2 .. 3 mesh widths
    size_big = w * rng.uniform(1.2, 3.0, (count, 2))
    r[big, 0:2] = (centre - 0.5 * size_big)[big]
    r[big, 2:4] = (centre + 0.5 * size_big)[big]
    pts = k % 13 == 5                                                           # points on x, every other one on z as well
    r[pts, 2] = r[pts, 0]
    both = pts & (k % 2 == 1)
    r[both, 3] = r[both, 1]
    rev = k % 7 == 2                                                            # reversed ends, x / z / both in turn
    rx, rz = rev & (k % 3 != 1), rev & (k % 3 != 0)
    r[rx, 0], r[rx, 2] = r[rx, 2].copy(), r[rx, 0].copy()
    r[rz, 1], r[rz, 3] = r[rz, 3].copy(), r[rz, 1].copy()
    far = k % 5 == 4                                                            # whole mesh periods towards negative coordinates
    r[far, 0] -= 3.0 * w; r[far, 2] -= 3.0 * w
    r[far & (k % 2 == 0), 1] -= 5.0 * w; r[far & (k % 2 == 0), 3] -= 5.0 * w
    aligned = node_rects(grid, vd, n)[0].astype(np.float64)                     # rows 400 .. (n = 16: 484): node_rects, as they are
    r[400:400 + len(aligned)] = aligned
    return r.astype(np.float32)


def planes_for(grid, vd):
    """Four planes of a frustum-like wedge over a mesh of width W, in an order that lets a later plane be reached or not: x >= -0.3 W,
    x <= 0.45 W, z >= -0.1 W, and y <= 1000, which everything satisfies."""
    w = abs(grid * vd)
    return np.array([[1.0, 0.0, 0.0, 0.3 * w], [-1.0, 0.0, 0.0, 0.45 * w], [0.0, 0.0, 1.0, 0.1 * w], [0.0, -1.0, 0.0, 1000.0]], np.float32)


def surfaces():
    """(tag, first_tile, cascades, uv_scales, grid, vertex_distance): the cascade sets of crafted_maps.VERTEX_CASCADE_SETS on the reference
    mesh with the uv bases in rotation, crafted_maps.geometries(), and one set with a negative uv_scale."""
    out = []
    for k, (first, count) in enumerate(CM.VERTEX_CASCADE_SETS):
        base = CM.VERTEX_UV_SCALES[k % len(CM.VERTEX_UV_SCALES)]
        out.append((f"tiles {first}..{first + count - 1} base {base}", first, count, CM.scales(first, count, base), CM.GRID, CM.VD))
    out += list(CM.geometries())
    out.append(("a negative uv_scale", 0, 3, [1.0, -0.61, 2.2], CM.GRID, CM.VD))
    return out


def cases():
    """(tag, first_tile, cascades, uv_scales, grid, vertex_distance, pad, with_planes): every surface with the pads in rotation, planes on
    every other one -- and each of the first three surfaces with every pad."""
    out = []
    for k, (tag, first, count, sc, grid, vd) in enumerate(surfaces()):
        out.append((tag, first, count, sc, grid, vd, PADS[k % len(PADS)], k % 2 == 0))
    for k, (tag, first, count, sc, grid, vd) in enumerate(surfaces()[:3]):
        for pad in PADS:
            if pad != PADS[k % len(PADS)]:
                out.append((tag, first, count, sc, grid, vd, pad, k % 2 == 1))
    return out


# ---- what tests/test_chain_readers_sizes_gpu.py runs on a real sea of 256^2 tiles (tests/lod.py: SIZES_N, SIZES_TILES) ----------------------
# Eight levels: node offsets beyond level 4, levels the builder's second launch writes, w >= N at 256, pads wider than a tile.
SIZES_RECTS = 2051                  # fills neither the last wave nor the last block; rows 400 .. 740 are node_rects(n = 256)
SIZES_PADS = (0, 1, 64, 300, 65536)             # none, the vertex stage's, 2^(L+1) of level 5, wider than the tile, the largest accepted
SIZES_FIRST_LEVELS = (1, 4, 8)                  # all stored, the common culling set, the top alone


def sizes_surfaces():
    """(tag, first_tile, cascades, uv_scales, grid, vertex_distance) on six tiles of crafted_maps.LENGTHS."""
    sets = ((0, 1, 1.0), (0, 3, 0.37), (2, 3, 2.5), (1, 5, 1.0))
    out = [(f"tiles {first}..{first + count - 1} base {base}", first, count, CM.scales(first, count, base), CM.GRID, CM.VD) for first, count, base in sets]
    out.append(("free uv_scales", 0, 3, [1.0, 2.7, 0.37], CM.GRID, CM.VD))
    out.append(("a negative uv_scale", 0, 3, [1.0, -0.61, 2.2], CM.GRID, CM.VD))
    out.append(("grid 513, tiles 3..5", 3, 3, CM.scales(3, 3), 513, CM.VD))
    return out


def sizes_cases():
    """(tag, first_tile, cascades, uv_scales, grid, vertex_distance, pad, with_planes): every surface with the pads in rotation, planes on
    every other one -- and the second surface with every other pad, planes the other way round."""
    out = []
    for k, (tag, first, count, sc, grid, vd) in enumerate(sizes_surfaces()):
        out.append((tag, first, count, sc, grid, vd, SIZES_PADS[k % len(SIZES_PADS)], k % 2 == 0))
    tag, first, count, sc, grid, vd = sizes_surfaces()[1]
    out += [(tag, first, count, sc, grid, vd, pad, True) for pad in SIZES_PADS if pad != SIZES_PADS[1]]
    return out


# The guarantee at a real size, on the device and in numpy (tests/test_bounds.py): rest points inside a rectangle, evaluated forward at mip
# level L, against the rectangle's box at pad_texels = 2^(L+1) as include/ocean_consumers.h tells such a caller (level 0: pad 0).
CONTAIN_RECTS, CONTAIN_POINTS, CONTAIN_SEED = 2000, 9, 20263
CONTAIN_SCALES = (1.0, 2.7, 0.37)               # three cascades from tile 0, free uv_scales
CONTAIN_LEVELS = (0, 1, 3, 5, 8)


def containment_inputs(grid, vd, n):
    """(rects [CONTAIN_RECTS, 4], xz [CONTAIN_RECTS * CONTAIN_POINTS, 2]): rect_set for tiles of n^2 -- wrapped, negative and reversed ones
    among them --, and per rectangle its two named corners and seven seeded points between them, clamped to the rectangle in fp32."""
    rects = rect_set(grid, vd, CONTAIN_RECTS, n=n)
    assert np.isfinite(rects).all()
    s = np.random.default_rng(CONTAIN_SEED).uniform(0.0, 1.0, (CONTAIN_RECTS, CONTAIN_POINTS, 2))
    s[:, 0], s[:, 1] = 0.0, 1.0
    r = rects.astype(np.float64)
    x = (r[:, None, 0] + (r[:, 2] - r[:, 0])[:, None] * s[..., 0]).astype(np.float32)
    z = (r[:, None, 1] + (r[:, 3] - r[:, 1])[:, None] * s[..., 1]).astype(np.float32)
    x = np.clip(x, np.minimum(rects[:, 0], rects[:, 2])[:, None], np.maximum(rects[:, 0], rects[:, 2])[:, None])
    z = np.clip(z, np.minimum(rects[:, 1], rects[:, 3])[:, None], np.maximum(rects[:, 1], rects[:, 3])[:, None])
    return rects, np.stack([x, z], axis=-1).reshape(-1, 2)


def containment_query(level):
    """(footprint, max_level, pad_texels) that put every cascade on `level` with t == 0, and the pad the header prescribes for it."""
    return (0.0, 0, 0) if level == 0 else (np.inf, level, 2 ** (level + 1))


def containment_excess(pos, lo, hi, e):
    """(largest excess of a position over its rectangle's box on x, y or z; largest lo.w - w) of the positions pos [rects * CONTAIN_POINTS, 4]
    -- negative: that far inside --, after asserting that every position lies in [lo - e, hi + e] and that its w is at least lo.w - e_w."""
    p = np.asarray(pos, dtype=np.float64).reshape(len(lo), CONTAIN_POINTS, 4)
    lo, hi = np.asarray(lo, dtype=np.float64)[:, None], np.asarray(hi, dtype=np.float64)[:, None]
    assert np.isfinite(p).all() and np.isfinite(lo).all() and np.isfinite(hi[..., :3]).all()
    over = np.maximum(p[..., :3] - hi[..., :3], lo[..., :3] - p[..., :3])
    over_w = lo[..., 3] - p[..., 3]
    bad = (over > e[:3]).any(axis=2) | (over_w > e[3])
    worst = float(over.max()), float(over_w.max())
    assert not bad.any(), f"{int(bad.sum())} positions outside their box, the first in rectangle {np.nonzero(bad.any(axis=1))[0][0]}; largest excess {worst[0]:.3e}, of w {worst[1]:.3e}; slack {e.tolist()}"
    return worst
