"""The surface bounds' restatement (tests/bounds.py) on the CPU: the pyramid against numpy's min / max of the blocks, the patch query's
guarantee by brute force against the level-0 forward evaluation of tests/lod.py -- and the vetting of what tests/test_patch_bounds_gpu.py
runs: its rectangles reach every branch of the level rule, the node rule and the classification.  No device.

The slack of the guarantee.  A bilinear sample is (c00*ia + c10*a)*ib + (c01*ia + c11*a)*b with ia = 1 - a, ib = 1 - b in fp32.  With exact
weights it is a convex combination of the four texels and cannot exceed the largest, M = max|texel| bounding them all.  a = s - floor(s) is
exact; ia = 1 - a is exact for a >= 0.5 and inexact by at most half an ulp of a number below 1, 2^-25, for a < 0.5 -- so the two weights
of an axis sum to at most 1 + 2^-25.  Five rounded operations follow on the way to the result (product, sum, product, product -- the
second bracket runs beside the first --, sum), each within a relative 2^-24.  Together: at most M * ((1 + 2^-25)^2 * (1 + 2^-24)^5 - 1)
< M * 2^-21 above the largest texel read, and as much below the smallest.  The largest texel read is at most the node maximum, because
both texels of either axis lie in the index range (tests/bounds.py: axis_range; t is monotone in p).  Summing the cascades adds nothing
beyond the sum of these slacks: the forward evaluation and the query add their terms in the same order from 0.0f, fp32 addition and the
product with A_c > 0 are monotone, so term-wise smaller inputs give a smaller or equal sum, and the slack of every term passes through
at most unchanged in size (up to its own rounding, far below the factor of more than 2 left in 2^-21).  Hence
e = 2^-21 * sum_c max|texel_c| (times A_c for y), and for the Jacobian slot, a minimum and not a sum, 2^-21 * max_c max|w texel|."""
import numpy as np
import pytest

import bounds as B
import crafted_maps as CM
import lod as L

F = np.float32


@pytest.fixture(scope="module")
def maps():
    return CM.maps()


def test_pyramid_nodes_are_the_min_and_max_of_their_blocks(maps):
    disp, _ = maps
    for tile in (0, 5):
        pyr = B.pyramid(disp[tile])
        assert [lo.shape for lo, _ in pyr] == [(8, 8, 4), (4, 4, 4), (2, 2, 4), (1, 1, 4)]
        for l, (lo, hi) in enumerate(pyr, start=1):
            s = 1 << l
            blocks = disp[tile].reshape(CM.N // s, s, CM.N // s, s, 4)
            assert np.array_equal(lo, blocks.min(axis=(1, 3))) and np.array_equal(hi, blocks.max(axis=(1, 3))), (tile, l)
            assert lo.dtype == np.float32 and np.all(lo <= hi)


def test_a_rectangle_that_is_exactly_one_node_gets_that_blocks_min_and_max(maps):
    """Non-vacuity: the bounds are not merely loose enough to contain everything."""
    disp, _ = maps
    rects, level, ny, nx = B.node_rects()
    assert len(rects) == 64 + 16 + 4 + 1 and np.array_equal(rects.astype(np.float64), B.node_rects()[0])
    amp = CM.CPU_AMPS[0]
    lo, hi, seen, _ = B.patch_bounds(disp[:1], [amp], [1.0], CM.GRID, CM.VD, rects, detail=True)
    d = seen[0]
    assert np.array_equal(d["level"], level)
    assert np.array_equal(d["nx0"], nx) and np.array_equal(d["nx1"], nx) and np.array_equal(d["nz0"], ny) and np.array_equal(d["nz1"], ny)
    assert np.array_equal(d["i1x"] - d["i0x"] + 1, 1 << level) and np.array_equal(d["i0x"], nx << level)
    for r in range(len(rects)):
        s = 1 << level[r]
        block = disp[0][ny[r] * s:(ny[r] + 1) * s, nx[r] * s:(nx[r] + 1) * s].reshape(-1, 4)
        mn, mx = block.min(axis=0), block.max(axis=0)
        x_lo, z_lo, x_hi, z_hi = min(rects[r, 0], rects[r, 2]), min(rects[r, 1], rects[r, 3]), max(rects[r, 0], rects[r, 2]), max(rects[r, 1], rects[r, 3])
        assert np.array_equal(lo[r], np.array([x_lo + mn[0], F(0) + mn[1] * F(amp), z_lo + mn[2], mn[3]], np.float32)), r
        assert np.array_equal(hi[r], np.array([x_hi + mx[0], F(0) + mx[1] * F(amp), z_hi + mx[2], 1.0], np.float32)), r


def test_the_level_rule_at_its_edges(maps):
    """w == N - 1 takes the level the rule gives, w == N the whole-tile node; first_level raises a level and never the whole-tile one; a
    negative index wraps; pad widens both ends."""
    disp, _ = maps
    p = lambda t: ((t + 0.5) / CM.N * CM.GRID - CM.GRID // 2) * CM.VD
    rects = np.array([[p(0.25), p(0.25), p(13.25), p(0.25)],            # i 0 .. 14: w = 15
                      [p(0.25), p(0.25), p(14.25), p(0.25)],            # i 0 .. 15: w = 16
                      [p(-1.75), p(2.25), p(-0.75), p(2.25)],           # i -2 .. 0: w = 3, level 2, nodes 3 and 0 on x
                      [p(3.25), p(3.25), p(3.25), p(3.25)],             # i 3 .. 4: w = 2, level 1, nodes 1 and 2
                      [p(2.25), p(2.25), p(2.25), p(2.25)]], np.float32)  # i 2 .. 3: level 1, node 1 alone
    _, _, seen, _ = B.patch_bounds(disp[:1], [1.0], [1.0], CM.GRID, CM.VD, rects, detail=True)
    d = seen[0]
    assert d["w"].tolist() == [15, 16, 3, 2, 2] and d["whole"].tolist() == [False, True, False, False, False]
    assert d["level"].tolist() == [4, 4, 2, 1, 1]
    assert (d["i0x"][2], d["i1x"][2], d["nx0"][2], d["nx1"][2]) == (-2, 0, 3, 0)
    assert (d["nx0"][3], d["nx1"][3], d["nx0"][4], d["nx1"][4]) == (1, 2, 1, 1)
    _, _, seen, _ = B.patch_bounds(disp[:1], [1.0], [1.0], CM.GRID, CM.VD, rects, first_level=3, detail=True)
    assert seen[0]["level"].tolist() == [4, 4, 3, 3, 3]
    assert (seen[0]["nx0"][2], seen[0]["nx1"][2]) == (1, 0)
    _, _, seen, _ = B.patch_bounds(disp[:1], [1.0], [1.0], CM.GRID, CM.VD, rects, pad=4, detail=True)
    assert seen[0]["w"].tolist() == [23, 24, 11, 10, 10] and seen[0]["level"].tolist() == [4, 4, 4, 4, 4]
    # a rectangle that is not finite: the whole-tile node, whatever the indices come to
    bad = rects.copy(); bad[3, 2] = np.nan; bad[4, 1] = np.inf
    lo, hi, seen, _ = B.patch_bounds(disp[:1], [1.0], [1.0], CM.GRID, CM.VD, bad, detail=True)
    assert seen[0]["whole"].tolist() == [False, True, False, True, True] and seen[0]["level"].tolist() == [4, 4, 2, 4, 4]
    # 0 means 1
    a = B.patch_bounds(disp[:1], [1.0], [1.0], CM.GRID, CM.VD, rects, first_level=0)
    b = B.patch_bounds(disp[:1], [1.0], [1.0], CM.GRID, CM.VD, rects, first_level=1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_classification_walks_the_planes_in_order():
    lo = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [-9, -1, -1, 0]], np.float32)
    hi = np.array([[1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0], [-8, 1, 1, 0]], np.float32)
    inside, cut, out = [1, 0, 0, 0.5], [1, 0, 0, -0.5], [-1, 0, 0, -2.0]
    assert B.classify(lo, hi, None).tolist() == [1, 1, 1, 1]
    assert B.classify(lo[:1], hi[:1], [inside]).tolist() == [2] and B.classify(lo[:1], hi[:1], [cut]).tolist() == [1]
    assert B.classify(lo[:1], hi[:1], [out]).tolist() == [0]
    cls, stop = B.classify(lo, hi, [cut, inside, out, cut], detail=True)
    assert cls.tolist() == [0, 0, 0, 0] and stop.tolist() == [2, 2, 2, 0]       # (the last row is outside the first plane already)
    cls, stop = B.classify(lo, hi, [inside, cut, inside], detail=True)
    assert cls.tolist() == [1, 1, 1, 0] and stop.tolist() == [-1, -1, -1, 0]
    # a zero coefficient takes the `hi` corner for far and the `lo` corner for near, as a >= 0 says
    assert B.classify(lo[:1], hi[:1], [[0, 0, -1, 0.5]]).tolist() == [1] and B.classify(lo[:1], hi[:1], [[0, 1, 0, 0]]).tolist() == [2]


def test_the_gpu_inputs_reach_every_branch(maps):
    disp, _ = maps
    reached = {f"level {l}": 0 for l in (1, 2, 3, 4)}
    reached.update({"one node on x": 0, "two nodes on x": 0, "one node on z": 0, "two nodes on z": 0, "negative index": 0, "w == N - 1": 0,
                    "w == N": 0, "w > N": 0, "first_level clamp": 0, "class 0": 0, "class 1": 0, "class 2": 0, "early stop": 0})
    pads, firsts = set(), set()
    for first_level in B.FIRST_LEVELS:
        for tag, first, count, sc, grid, vd, pad, with_planes in B.cases():
            sl = slice(first, first + count)
            rects = B.rect_set(grid, vd)
            assert rects.shape == (B.RECTS, 4) and np.isfinite(rects).all()
            planes = B.planes_for(grid, vd) if with_planes else None
            lo, hi, seen, stop = B.patch_bounds(disp[sl], CM.CPU_AMPS[sl], sc, grid, vd, rects, first_level, pad, planes, detail=True)
            assert np.isfinite(lo).all() and np.isfinite(hi).all() and np.all(lo[:, :3] <= hi[:, :3]), tag
            pads.add(pad); firsts.add(first_level)
            plain = B.patch_bounds(disp[sl], CM.CPU_AMPS[sl], sc, grid, vd, rects, 1, pad)[0] if first_level > 1 else None
            for c, d in enumerate(seen):
                inside = ~d["whole"]
                if first_level == 1:
                    for l in (1, 2, 3, 4):
                        reached[f"level {l}"] += int((inside & (d["level"] == l)).sum())
                reached["one node on x"] += int((inside & (d["nx0"] == d["nx1"])).sum())
                reached["two nodes on x"] += int((inside & (d["nx0"] != d["nx1"])).sum())
                reached["one node on z"] += int((inside & (d["nz0"] == d["nz1"])).sum())
                reached["two nodes on z"] += int((inside & (d["nz0"] != d["nz1"])).sum())
                reached["negative index"] += int((inside & ((d["i0x"] < 0) | (d["i0z"] < 0))).sum())
                reached["w == N - 1"] += int((d["w"] == CM.N - 1).sum())
                reached["w == N"] += int((d["w"] == CM.N).sum())
                reached["w > N"] += int((d["w"] > CM.N).sum())
                assert np.all(d["level"] >= first_level) and np.all(d["level"] <= 4)
                assert np.all((d["i1x"] - d["i0x"] + 1 <= (1 << d["level"])) | d["whole"])
            if plain is not None:
                reached["first_level clamp"] += int((plain != lo).any(axis=1).sum())
                assert np.all(lo[:, :3] <= plain[:, :3])                # a coarser level can only widen the box
            if with_planes:
                for k in (0, 1, 2):
                    reached[f"class {k}"] += int((hi[:, 3] == k).sum())
                # the early stop: a row that stopped at a plane and that a LATER plane, looked at alone, would call a straddle
                for k in range(len(planes) - 1):
                    later = np.zeros(len(rects), bool)
                    for j in range(k + 1, len(planes)):
                        later |= B.classify(lo, hi, planes[j:j + 1]) == 1
                    reached["early stop"] += int(((stop == k) & later).sum())
            else:
                assert np.all(hi[:, 3] == 1)
    assert all(v > 0 for v in reached.values()), reached
    assert pads == set(B.PADS) and firsts == set(B.FIRST_LEVELS)
    tags = [c[0] for c in B.cases()]
    assert len([t for t in tags if t.startswith("tiles ")]) >= len(CM.VERTEX_CASCADE_SETS) and "a negative uv_scale" in tags
    assert {g[0] for g in CM.geometries()} <= set(tags)


def test_the_rectangle_set_has_what_its_docstring_says():
    r = B.rect_set(CM.GRID, CM.VD).astype(np.float64)
    w = CM.GRID * CM.VD
    assert len(r) == B.RECTS == 4099 and B.RECTS % 64 != 0 and B.RECTS % 256 != 0
    assert ((r[:, 0] == r[:, 2]) & (r[:, 1] != r[:, 3])).sum() > 50 and ((r[:, 0] == r[:, 2]) & (r[:, 1] == r[:, 3])).sum() > 50
    assert (r[:, 0] > r[:, 2]).sum() > 100 and (r[:, 1] > r[:, 3]).sum() > 100
    assert (np.abs(r[:, 2] - r[:, 0]) > w).sum() > 100
    assert (np.maximum(r[:, 0], r[:, 2]) < -w).sum() > 100 and (np.maximum(r[:, 1], r[:, 3]) < -2 * w).sum() > 100
    aligned = B.node_rects()[0]
    assert np.array_equal(B.rect_set(CM.GRID, CM.VD)[400:400 + len(aligned)], aligned)


@pytest.mark.parametrize("case", [c for c in B.cases() if c[6] == 0][:4] + [c for c in B.cases() if c[6] != 0][:3], ids=lambda c: f"{c[0]} pad {c[6]}")
@pytest.mark.parametrize("first_level", B.FIRST_LEVELS)
def test_every_rest_point_of_a_rectangle_lands_inside_its_box(maps, case, first_level):
    """Brute force: 23 x 23 rest points per rectangle through the level-0 forward evaluation (tests/lod.py at footprint 0)."""
    disp, nrm = maps
    tag, first, count, sc, grid, vd, pad, _ = case
    sl = slice(first, first + count)
    rects = B.rect_set(grid, vd)[::9]
    lo, hi = B.patch_bounds(disp[sl], CM.CPU_AMPS[sl], sc, grid, vd, rects, first_level, pad)
    e = B.slack(disp[sl], CM.CPU_AMPS[sl])
    s = np.linspace(0.0, 1.0, 23)
    worst = 0.0
    for r, (x0, z0, x1, z1) in enumerate(rects.astype(np.float64)):
        # points between the ends, the ends themselves in fp32 exactly
        xs = np.clip((x0 + (x1 - x0) * s).astype(np.float32), min(rects[r, 0], rects[r, 2]), max(rects[r, 0], rects[r, 2]))
        zs = np.clip((z0 + (z1 - z0) * s).astype(np.float32), min(rects[r, 1], rects[r, 3]), max(rects[r, 1], rects[r, 3]))
        gx, gz = [a.ravel() for a in np.meshgrid(xs, zs)]
        xzf = np.stack([gx, gz, np.zeros_like(gx)], axis=1)
        pos, _ = L.sample_surface_lod(disp[sl], nrm[sl], CM.CPU_AMPS[sl], sc, grid, vd, L.CHOPPY, xzf)
        p = pos.astype(np.float64)
        over = max((p[:, :3] - hi[r, :3]).max(), (lo[r, :3] - p[:, :3]).max(), (lo[r, 3] - p[:, 3]).max())
        worst = max(worst, over)
        assert np.all(p[:, :3] <= hi[r, :3] + e[:3]) and np.all(p[:, :3] >= lo[r, :3] - e[:3]), (tag, r, rects[r])
        assert np.all(p[:, 3] >= lo[r, 3] - e[3]), (tag, r)
    print(f"{tag} pad {pad} first_level {first_level}: largest excess over the box {worst:.3e} (slack {e.tolist()})")


# ---- the inputs of tests/test_chain_readers_sizes_gpu.py: tiles of 256^2 ---------------------------------------------------------------------
def test_the_generators_give_the_16_squared_inputs_unchanged_at_their_defaults():
    """The n parameter's default is the crafted maps' size: the rectangle set of tests/test_patch_bounds_gpu.py is, byte for byte, what the
    generator gave before it took an n (the digest is of that array), and spelling the default out changes nothing."""
    import hashlib
    rects = B.rect_set(CM.GRID, CM.VD)
    assert hashlib.sha256(rects.tobytes()).hexdigest() == "893517e1c3889052b6ad4280693fa40b1ddcaa1686b05942e3107a874000a72f"
    assert np.array_equal(B.rect_set(CM.GRID, CM.VD, n=16).view(np.uint32), rects.view(np.uint32))
    assert all(np.array_equal(a, b) for a, b in zip(B.node_rects(), B.node_rects(n=16)))


@pytest.fixture(scope="module")
def maps256():
    return L.random_maps(L.SIZES_N, L.SIZES_TILES, 20262)


def test_the_256_rectangle_set_has_what_its_docstring_says(maps256):
    disp, _ = maps256
    n, top = L.SIZES_N, 8
    rects, level, ny, nx = B.node_rects(n=n)
    assert np.bincount(level).tolist() == [0, 64, 64, 64, 64, 64, 16, 4, 1] and np.array_equal(rects.astype(np.float64), B.node_rects(n=n)[0])
    assert all(len({(y, x) for y, x in zip(ny[level == l], nx[level == l])}) == (level == l).sum() for l in range(1, top + 1))
    # each is exactly its node: the block's own minimum and maximum, at offsets beyond those of a 16^2 chain
    lo, hi, seen, _ = B.patch_bounds(disp[:1], [1.0], [1.0], CM.GRID, CM.VD, rects, detail=True)
    d = seen[0]
    assert np.array_equal(d["level"], level) and np.array_equal(d["nx0"], nx) and np.array_equal(d["nx1"], nx)
    assert np.array_equal(d["nz0"], ny) and np.array_equal(d["nz1"], ny) and np.array_equal(d["i0x"], nx << level)
    for r in range(len(rects)):
        s = 1 << level[r]
        block = disp[0][ny[r] * s:(ny[r] + 1) * s, nx[r] * s:(nx[r] + 1) * s].reshape(-1, 4)
        assert np.array_equal(lo[r, 1::2], block.min(axis=0)[1::2]) and np.array_equal(hi[r, 1], block.max(axis=0)[1]), r
    r = B.rect_set(CM.GRID, CM.VD, B.SIZES_RECTS, n=n).astype(np.float64)
    w = CM.GRID * CM.VD
    assert len(r) == B.SIZES_RECTS and B.SIZES_RECTS % 64 != 0 and B.SIZES_RECTS % 256 != 0 and np.isfinite(r).all()
    assert np.array_equal(r[400:400 + len(rects)], rects.astype(np.float64)) and 400 + len(rects) < B.SIZES_RECTS
    size = np.abs(r[:, 2:] - r[:, :2]).max(axis=1) / (w / n)                   # in texels of tile 0
    assert (size[size > 0] < 0.25).sum() > 10 and all(((size > 2.0 ** k) & (size <= 2.0 ** (k + 1))).sum() > 50 for k in range(0, 8))
    assert ((size > n) & (size <= 1.25 * n)).sum() > 10 and (size > 1.25 * n).sum() > 100
    assert (r[:, 0] > r[:, 2]).sum() > 50 and (r[:, 1] > r[:, 3]).sum() > 50 and (np.maximum(r[:, 0], r[:, 2]) < -w).sum() > 50


def test_the_256_inputs_reach_every_branch(maps256):
    """What test_the_gpu_inputs_reach_every_branch asks of the 16^2 inputs, and every level first_level .. 8 for each first_level."""
    disp, _ = maps256
    n, top = L.SIZES_N, 8
    keys = ["one node on x", "two nodes on x", "one node on z", "two nodes on z", "negative index", "w == N - 1", "w == N", "w > N",
            "first_level clamp", "class 0", "class 1", "class 2", "early stop", "pad beyond a tile", "index beyond 2^16"]
    reached = dict.fromkeys(keys, 0)
    pads = set()
    for first_level in B.SIZES_FIRST_LEVELS:
        levels = np.zeros(top + 1, np.int64)
        for tag, first, count, sc, grid, vd, pad, with_planes in B.sizes_cases():
            sl = slice(first, first + count)
            rects = B.rect_set(grid, vd, B.SIZES_RECTS, n=n)
            planes = B.planes_for(grid, vd) if with_planes else None
            lo, hi, seen, stop = B.patch_bounds(disp[sl], CM.CPU_AMPS[sl], sc, grid, vd, rects, first_level, pad, planes, detail=True)
            assert np.isfinite(lo).all() and np.isfinite(hi).all() and np.all(lo[:, :3] <= hi[:, :3]), tag
            pads.add(pad)
            plain = B.patch_bounds(disp[sl], CM.CPU_AMPS[sl], sc, grid, vd, rects, 1, pad)[0] if first_level > 1 else None
            for d in seen:
                inside = ~d["whole"]
                levels += np.bincount(d["level"][inside], minlength=top + 1)
                reached["one node on x"] += int((inside & (d["nx0"] == d["nx1"])).sum())
                reached["two nodes on x"] += int((inside & (d["nx0"] != d["nx1"])).sum())
                reached["one node on z"] += int((inside & (d["nz0"] == d["nz1"])).sum())
                reached["two nodes on z"] += int((inside & (d["nz0"] != d["nz1"])).sum())
                reached["negative index"] += int((inside & ((d["i0x"] < 0) | (d["i0z"] < 0))).sum())
                reached["w == N - 1"] += int((d["w"] == n - 1).sum())
                reached["w == N"] += int((d["w"] == n).sum())
                reached["w > N"] += int((d["w"] > n).sum())
                reached["pad beyond a tile"] += int(pad >= n)
                reached["index beyond 2^16"] += int((np.abs(d["i0x"]) > 65536).sum())
                assert np.all(d["level"] >= first_level) and np.all(d["level"] <= top)
                assert np.all((d["i1x"] - d["i0x"] + 1 <= (1 << d["level"])) | d["whole"])
            if plain is not None:
                reached["first_level clamp"] += int((plain != lo).any(axis=1).sum())
                assert np.all(lo[:, :3] <= plain[:, :3])
            if with_planes:
                for k in (0, 1, 2):
                    reached[f"class {k}"] += int((hi[:, 3] == k).sum())
                for k in range(len(planes) - 1):
                    later = np.zeros(len(rects), bool)
                    for j in range(k + 1, len(planes)):
                        later |= B.classify(lo, hi, planes[j:j + 1]) == 1
                    reached["early stop"] += int(((stop == k) & later).sum())
            else:
                assert np.all(hi[:, 3] == 1)
        # (the whole-tile node a rule gives, not one forced by w >= N: level 8 is reached by w in 129 .. 255 too)
        assert np.all(levels[first_level:] > 0) and np.all(levels[:first_level] == 0), (first_level, levels)
    assert all(v > 0 for v in reached.values()), reached
    assert pads == set(B.SIZES_PADS) and {c[7] for c in B.sizes_cases() if c[6] == 0} == {True, False}
    assert all(c[1] + c[2] <= L.SIZES_TILES for c in B.sizes_cases())


def test_forward_evaluations_at_mip_level_L_stay_inside_the_box_padded_by_two_to_the_L_plus_one(maps256):
    """include/ocean_consumers.h: a caller "who samples at mip level L sets pad_texels = 2^(L+1)".  With s = u N - 0.5 the level-0
    texel coordinate, the level-L sample reads the two level-L texels j, j + 1 with j = floor((s + 0.5) / 2^L - 0.5), whose blocks are the
    level-0 texels j 2^L .. (j + 2) 2^L - 1: from less than 1.5 * 2^L below s to less than 1.5 * 2^L above it, inside floor(s) - pad ..
    floor(s) + 1 + pad.  A mip texel is a mean formed by monotone rounding and lies between its block's extremes, and t == 0 adds no blend:
    B.slack as it stands.  The same check runs on the device in tests/test_chain_readers_sizes_gpu.py."""
    disp, nrm = maps256
    n, sc, amps = L.SIZES_N, list(B.CONTAIN_SCALES), CM.CPU_AMPS[:3]
    rects, xz = B.containment_inputs(CM.GRID, CM.VD, n)
    assert len(rects) == 2000 and len(xz) == 18000
    e = B.slack(disp[:3], amps)
    for level in B.CONTAIN_LEVELS:
        f, max_level, pad = B.containment_query(level)
        xzf = np.concatenate([xz, np.full((len(xz), 1), f, np.float32)], axis=1)
        pos, out_nrm, seen = L.sample_surface_lod(disp[:3], nrm[:3], amps, sc, CM.GRID, CM.VD, L.CHOPPY, xzf, 1.0, max_level, detail=True)
        assert all(np.all(lev == level) and np.all(t == 0) for lev, t in seen)
        lo, hi = B.patch_bounds(disp[:3], amps, sc, CM.GRID, CM.VD, rects, 1, pad)
        worst, worst_w = B.containment_excess(pos, lo, hi, e)
        print(f"level {level} pad {pad}: largest excess over a box {worst:.3e}, of w below its bound {worst_w:.3e} (slack {e.tolist()})")
    # the check sees a box that is not the rectangle's own: its neighbour's in the list
    with pytest.raises(AssertionError):
        B.containment_excess(pos, np.roll(lo, 1, axis=0), np.roll(hi, 1, axis=0), e)
