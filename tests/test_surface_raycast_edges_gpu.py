"""The ray-cast kernel (k_raycast_surface) at its edges on the MI355X: every (steps, refine) path of the wave-uniform loop, ray counts that
leave a lane group, a wave or a block partly filled, wave-mates of every kind, the decision table of include/ocean_consumers.h asserted
on the kernel itself, vertical rays against the surface query, and a flat sea.  The comparison rules are those of
tests/test_surface_raycast_gpu.py (_rays, _batch_with_maps, _compare, imported unchanged); the restatement is tests/surface_raycast.py."""
import numpy as np
import pytest

import surface_raycast as R
from test_surface_raycast_gpu import LENGTHS3, _batch_with_maps, _compare, _rays

pytestmark = pytest.mark.gpu
F = np.float32
N, GRID, VD, K = 64, 512, 1000.0 / 512, 8
SCALES = [LENGTHS3[0] / L for L in LENGTHS3]
SEED = 0x5EED0000 + N
MISS = np.array([0.0, 0.0, 0.0, -1.0], np.float32)
SENTINEL = 0x7FC0BEEF               # a quiet NaN with a payload no result carries


def _status(hit):
    """0 hit, 1 miss, 2 under water."""
    return np.where(hit[:, 3] >= 0.0, 0, np.where(hit[:, 3] == -2.0, 2, 1))


def _bits(hit, nrm):
    return np.concatenate([hit, nrm], axis=1).view(np.uint32)


@pytest.fixture(scope="module")
def sea():
    """One context of three cascades at 64^2 and the restatement's surface on the maps read back from its frame."""
    b, amps, disp, nrm = _batch_with_maps(N, LENGTHS3, SEED)
    surf = R.Surface(list(disp), list(nrm), amps, [-1.0] * 3, LENGTHS3, SCALES, GRID, VD, -1.0, K)
    yield b, surf
    b.close()


def _cast(b, rays, max_distance, steps=0, refine=0):
    return b.raycast_surface(rays[:, :3], rays[:, 3:], max_distance, steps, refine, 0, SCALES, GRID, VD, -1.0, K)


def _cast_device(b, d_rays_ptr, count, max_distance, steps=0, refine=0, sentinel_rows=64):
    """The device variant into outputs of count + sentinel_rows rows pre-filled with a bit pattern: (hit, nrm) of the whole allocation."""
    import torch
    rows = count + sentinel_rows
    d_hit = torch.full((rows, 4), SENTINEL, dtype=torch.int32, device="cuda")
    d_nrm = torch.full((rows, 4), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    b.raycast_surface_device(d_rays_ptr, count, d_hit.data_ptr(), d_nrm.data_ptr(), max_distance, steps, refine, 0, SCALES, GRID, VD, -1.0, K)
    b.synchronize()
    return d_hit.cpu().numpy().view(np.uint32), d_nrm.cpu().numpy().view(np.uint32)


def mixed_rays(count, hmax, seed):
    """Half `camera`, half `random` (the camera frustum is a square number of rays; `random` fills up to count)."""
    cam = _rays("camera", count // 2, hmax, seed)
    return np.concatenate([cam, _rays("random", count - len(cam), hmax, seed + 1)])


SETTINGS = [(1, 1), (2, 3), (15, 1), (16, 2), (17, 8), (31, 3), (33, 1), (100, 8), (4096, 1)]


@pytest.mark.parametrize("steps,refine", SETTINGS)
def test_settings_matrix(sea, steps, refine):
    """Every way through the march (fewer samples than a lane group, exactly one group, one sample more, a partial last group, many
    groups) and through 1 .. 8 refinement rounds, against the restatement under the unchanged _compare: equal status on every ray, at
    least 99.9 % of the rays bit-identical, every other one a near-tie.  From refine = 4 on the bracket is so narrow that every hit's
    deciding samples lie within 1e-4 m of zero (all 3356 hits of a 4096-ray cast did), so the near-tie clause does not bind there: the
    99.9 % cap is the condition.  No setting is vacuous: at least 5 % of its rays hit and at least 5 % start under water."""
    b, surf = sea
    count = 256 if steps == 4096 else 2048          # the restatement evaluates all steps + 1 samples of every ray
    rays = mixed_rays(count, float(surf.hmax), 100 + steps)
    hit, nr = _cast(b, rays, 1500.0, steps, refine)
    ohit, onr, closest = R.raycast_surface(surf, rays, 1500.0, steps, refine, detail=True)
    counts = np.bincount(_status(hit), minlength=3)
    print(f"steps={steps} refine={refine}: hit/miss/under {counts.tolist()} of {count} (restatement {np.bincount(_status(ohit), minlength=3).tolist()})")
    same = _compare(hit, nr, ohit, onr, closest, (steps, refine))
    print(f"steps={steps} refine={refine}: {same}/{count} rays bit-identical")
    assert counts[0] >= 0.05 * count and counts[2] >= 0.05 * count, counts


def test_tails(sea):
    """Ray counts that leave the last lane group's wave-mates, the last wave and the last block without a ray: the first `count` rays
    of a 300-ray call alone give the same bits; the device variant writes those rows and not one float beyond them; and rays that are
    only 4-byte aligned (the header's promise) give the same bits again."""
    import torch
    b, surf = sea
    rays = mixed_rays(300, float(surf.hmax), 7)
    hit, nr = _cast(b, rays, 1500.0)
    assert np.bincount(_status(hit), minlength=3).min() > 0
    whole = _bits(hit, nr)
    d_rays = torch.from_numpy(rays).cuda()
    d_shifted = torch.zeros(1 + rays.size, dtype=torch.float32, device="cuda")
    d_shifted[1:] = d_rays.reshape(-1)
    assert d_shifted.data_ptr() % 16 == 0
    for count in (1, 3, 4, 5, 15, 16, 17, 63, 255, 257):
        got = _bits(*_cast(b, rays[:count], 1500.0))
        assert np.array_equal(got, whole[:count]), (count, np.nonzero((got != whole[:count]).any(axis=1))[0])
        for ptr in (d_rays.data_ptr(), d_shifted.data_ptr() + 4):
            dh, dn = _cast_device(b, ptr, count, 1500.0)
            assert np.array_equal(np.concatenate([dh[:count], dn[:count]], axis=1), got), (count, ptr % 16)
            assert np.all(dh[count:] == np.uint32(SENTINEL)) and np.all(dn[count:] == np.uint32(SENTINEL)), (count, ptr % 16)


MATE_STEPS = 256                    # 17 group-wide steps of 16 samples: a ray that marches them all keeps its wave looping


def wave_mate_rays(b, surf, groups, seed=3):
    """4 * groups rays; every aligned group of four (the four lane groups of one wave) holds, in this order: a ray without a direction,
    an origin below the slab, a steep ray from just above the water (its hit is among the first 16 samples), and a grazing ray that
    marches to the end of its segment or to a far crest."""
    rng = np.random.default_rng(seed)
    hm = float(surf.hmax)
    rays = np.zeros((groups, 4, 6), np.float32)
    xz = rng.uniform(-500.0, 500.0, (groups, 4, 2)).astype(np.float32)
    rays[..., 0], rays[..., 2] = xz[..., 0], xz[..., 1]
    rays[:, 0, 1] = hm + rng.uniform(0.0, 20.0, groups)                                     # no direction: d = 0
    rays[:, 1, 1] = -hm - rng.uniform(0.0, 5.0, groups)                                     # below the slab
    rays[:, 1, 3:] = rng.normal(size=(groups, 3))
    pos, _ = b.query_surface(xz[:, 2], 0, SCALES, GRID, VD, -1.0, K)
    rays[:, 2, 1] = pos[:, 1] + F(0.02) * F(hm)                                             # steep, from 2 % of Hmax above the water
    pitch, yaw = rng.uniform(np.radians(60.0), np.radians(90.0), groups), rng.uniform(0.0, 2.0 * np.pi, groups)
    rays[:, 2, 3:] = np.stack([np.cos(pitch) * np.sin(yaw), -np.sin(pitch), np.cos(pitch) * np.cos(yaw)], axis=1)
    pos, _ = b.query_surface(xz[:, 3], 0, SCALES, GRID, VD, -1.0, K)
    rays[:, 3, 1] = pos[:, 1] + rng.uniform(5.0, 15.0, groups).astype(np.float32)           # grazing, from some metres above the water
    pitch, yaw = rng.uniform(np.radians(0.5), np.radians(4.0), groups), rng.uniform(0.0, 2.0 * np.pi, groups)
    rays[:, 3, 3:] = np.stack([np.cos(pitch) * np.sin(yaw), -np.sin(pitch), np.cos(pitch) * np.cos(yaw)], axis=1) * 2.5
    return rays.reshape(-1, 6)


def check_wave_mates(surf, rays, hit, max_distance, steps):
    """The four kinds are what they were built to be (from the header's rules and the returned t alone)."""
    st = _status(hit).reshape(-1, 4)
    assert np.all(st[:, 0] == 1) and np.all(st[:, 1] == 2) and np.all(st[:, 2] == 0), [int((st[:, k] != w).sum()) for k, w in enumerate((1, 2, 0))]
    o, d, _ = R.unit_rays(rays)
    t0, t1, _ = R.clip(surf, o, d, max_distance)
    t0, t1, t = t0.reshape(-1, 4), t1.reshape(-1, 4), hit[:, 3].reshape(-1, 4)
    first_step = t[:, 2] <= t0[:, 2] + F(15.0) * ((t1[:, 2] - t0[:, 2]) / F(steps))          # at or before sample 15
    assert first_step.mean() >= 0.95, float(first_step.mean())
    graze_hit = st[:, 3] == 0
    late = t[graze_hit, 3] > t0[graze_hit, 3] + F(16.0) * ((t1[graze_hit, 3] - t0[graze_hit, 3]) / F(steps))
    marched = (~graze_hit).sum() + late.sum()            # a miss took every sample, a late hit more than one group-wide step
    assert marched >= 0.9 * len(st) and graze_hit.sum() >= 0.05 * len(st) and (~graze_hit).sum() >= 0.05 * len(st), (int(marched), int(graze_hit.sum()))
    return int(first_step.sum()), int(graze_hit.sum()), int(late.sum())


def test_wave_mates_do_not_matter(sea):
    """Lane groups that are done at once (no direction, below the slab), after one step (a steep hit) and after all of them (a grazing
    ray) share every wave; a permutation gives every ray other wave-mates, and not a bit of its answer may change."""
    b, surf = sea
    rays = wave_mate_rays(b, surf, 1024)
    hit, nr = _cast(b, rays, 300.0, MATE_STEPS)
    early, graze_hits, late = check_wave_mates(surf, rays, hit, 300.0, MATE_STEPS)
    print(f"wave-mates: {early}/1024 steep hits in the first step; grazing rays: {graze_hits} hits ({late} after the first step), {1024 - graze_hits} misses")
    perm = np.random.default_rng(11).permutation(len(rays))
    assert (perm % 4 != np.arange(len(rays)) % 4).mean() > 0.5
    phit, pnr = _cast(b, rays[perm], 300.0, MATE_STEPS)
    assert np.array_equal(_bits(phit, pnr), _bits(hit, nr)[perm]), int((_bits(phit, pnr) != _bits(hit, nr)[perm]).any(axis=1).sum())


def table_rays(hm):
    """(rays, status): the eight rays of tests/test_surface_raycast.py::test_rays_that_miss and six more, for max_distance = 40, each
    with the status the header's rules give it (0 hit, 1 miss, 2 under water)."""
    hm = F(hm)
    h = float(hm)
    big, small = 1e30, 1e-30
    table = [
        ([0.0, h + 5.0, 0.0, 0.3, 1.0, 0.2], 1),                    # Slab, d.y > 0 above it: t1 < 0 = t0, empty
        ([10.0, h + 1e-3, -4.0, 0.0, 0.5, 0.0], 1),                 # the same from just above the slab
        ([0.0, h + 1.0, 0.0, 1.0, 0.0, 0.0], 1),                    # Slab, d.y == 0: empty unless o.y < Hmax
        ([5.0, h, 5.0, 0.0, 0.0, -2.0], 1),                         # ... and o.y == Hmax is not < Hmax
        ([0.0, h + 50.0, 0.0, 0.0, -1.0, 0.0], 1),                  # Slab, d.y < 0: t1 = max_distance = 40 < t0 = 50
        ([0.0, h + 50.0, 0.0, 0.0, 0.0, 0.0], 1),                   # Direction: len == 0
        ([0.0, h + 50.0, 0.0, np.inf, -1.0, 0.0], 1),               # Direction: len not finite
        ([0.0, h + 50.0, 0.0, np.nan, -1.0, 0.0], 1),
        ([0.0, h + 5.0, 0.0, big, -big, 0.0], 1),                   # Direction: dx * dx overflows, len = inf
        ([0.0, h + 5.0, 0.0, small, -small, 0.0], 1),               # Direction: dx * dx underflows to 0, len = 0
        ([0.0, np.nan, 0.0, 0.0, -1.0, 0.0], 1),                    # o.y NaN: not <= -Hmax; fmaxf / fminf drop it, t0 = 0, t1 = 40; no f <= 0
        ([20.0, -h, -30.0, 0.0, -1.0, 0.0], 2),                     # Slab: o.y <= -Hmax, the origin is under water
        ([20.0, float(np.nextafter(-hm, F(np.inf))), -30.0, 0.1, 1.0, 0.0], 2),      # March: t0 == 0 and f(t_0) <= 0, under water
        ([20.0, float(np.nextafter(hm, F(-np.inf))), -30.0, 1.0, 0.0, 1.0], 1),      # d.y == 0, o.y < Hmax: 40 m above every wave, no f <= 0
    ]
    rays = np.array([r for r, _ in table], np.float32)
    assert rays[11, 1] == -hm and -hm < rays[12, 1] < -hm * F(0.999) and hm * F(0.9999) < rays[13, 1] < hm and rays[1, 1] > hm
    return rays, np.array([s for _, s in table])


def test_the_headers_table_on_the_kernel(sea):
    """Direction, Slab and March of include/ocean_consumers.h on rays built to sit on each rule's edge: the status is the one the header's
    text gives (written out in table_rays), a miss is (0, 0, 0, -1) and zeros, an origin under water is the surface query at (o.x, o.z)
    with the depth o.y - P.y <= 0; and every ray equals the restatement."""
    b, surf = sea
    rays, want = table_rays(surf.hmax)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        hit, nr = _cast(b, rays, 40.0)
        ohit, onr, closest = R.raycast_surface(surf, rays, 40.0, detail=True)
    assert np.array_equal(_status(hit), want), (_status(hit), want)
    miss = want == 1
    assert np.array_equal(hit[miss], np.tile(MISS, (miss.sum(), 1))) and np.array_equal(nr[miss].view(np.uint32), np.zeros((miss.sum(), 4), np.uint32))
    under = want == 2
    pos, qn = b.query_surface(rays[under][:, [0, 2]], 0, SCALES, GRID, VD, -1.0, K)
    assert np.array_equal(hit[under, :3], pos[:, :3]) and np.all(hit[under, 3] == -2.0) and np.array_equal(nr[under, :3], qn[:, :3])
    assert np.array_equal(nr[under, 3], rays[under, 1] - pos[:, 1]) and np.all(nr[under, 3] <= 0.0)
    _compare(hit, nr, ohit, onr, closest, "table")
    hit, _ = _cast(b, rays[4:5], float(60.0 + 2.0 * surf.hmax))       # the vertical ray reaches the water once max_distance covers the slab
    assert hit[0, 3] > 50.0


@pytest.mark.parametrize("steps,refine", [(0, 0), (17, 1)])
def test_vertical_rays_hit_the_queried_height(sea, steps, refine):
    """Geometry without the restatement: along a vertical ray H is one number, so the hit is the surface query at (o.x, o.z), bit for bit,
    and t = o.y - P.y up to rounding (1e-4 m, the bound of the CPU property test; f is linear in t, so one refinement round does)."""
    b, surf = sea
    rng = np.random.default_rng(1)
    count = 2000
    xz = rng.uniform(-500.0, 500.0, (count, 2)).astype(np.float32)
    oy = (surf.hmax + rng.uniform(0.0, 30.0, count)).astype(np.float32)
    rays = np.zeros((count, 6), np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 4] = xz[:, 0], oy, xz[:, 1], -1.0
    hit, nr = _cast(b, rays, 200.0, steps, refine)
    pos, qn = b.query_surface(xz, 0, SCALES, GRID, VD, -1.0, K)
    assert np.all(hit[:, 3] >= 0.0), np.bincount(_status(hit), minlength=3)
    assert np.array_equal(hit[:, :3], pos[:, :3]) and np.array_equal(nr[:, :3], qn[:, :3])
    err = float(np.abs(hit[:, 3] - (oy - pos[:, 1])).max())
    print(f"vertical rays steps={steps} refine={refine}: |t - (o.y - P.y)| <= {err:.3g} m, |gap| <= {float(np.abs(nr[:, 3]).max()):.3g} m")
    assert err <= 1e-4


@pytest.fixture(scope="module")
def flat_sea():
    """phillips_const = 0 (tests/test_parity_gpu.py::test_zero_spectrum_minmax_quirk): every height 0, the amplitude FLT_MIN."""
    import watersurfacerendering_amd as W
    b = W.OceanBatch(32, 1, 0)
    b.set_params(phillips_const=0.0)
    b.prepare(1)
    amp = float(b.compute_waves(2.0)[0])
    assert amp == float(np.finfo(np.float32).tiny)
    yield b
    b.close()


@pytest.mark.parametrize("steps,refine", [(0, 0), (1, 1), (17, 8)])
def test_a_flat_sea_is_hit_by_every_downward_ray(flat_sea, steps, refine):
    """Calm water is a picking target: 4099 downward rays (a ray count that fills neither the last wave nor the last block) all meet the
    plane y = 0 with the normal (0, 1, 0), within the rounding bounds R.check_flat_sea derives.  Before the slab had its 1 mm floor about
    4 % of them missed.  The restatement's twin: tests/test_surface_raycast.py::test_a_flat_sea_is_hit_by_every_downward_ray."""
    rays = R.flat_sea_rays()
    assert len(rays) == 4099
    hit, nr = flat_sea.raycast_surface(rays[:, :3], rays[:, 3:], 400.0, steps, refine, 0, (1.0,), GRID, VD, -1.0, K)
    print(f"flat sea steps={steps} refine={refine}: hit/miss/under {np.bincount(_status(hit), minlength=3).tolist()}")
    gap_ulps, t_err = R.check_flat_sea(rays, hit, nr, (steps, refine))
    print(f"flat sea steps={steps} refine={refine}: gap <= {gap_ulps:.2f} ulp(o.y), t off by <= {t_err:.3g}")


def test_rays_at_the_surface_of_a_flat_sea(flat_sea):
    near = np.array([r for r, _ in R.NEAR_SURFACE], np.float32)
    R.check_near_surface(*flat_sea.raycast_surface(near[:, :3], near[:, 3:], 40.0, 0, 0, 0, (1.0,), GRID, VD, -1.0, K))
