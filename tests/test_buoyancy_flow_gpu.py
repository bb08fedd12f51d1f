"""Buoyancy with drag against the moving water on the MI355X (include/ocean_consumers.h: ocean_buoyancy_bodies_flow / _device): the
FLOW instantiation of k_buoyancy_bodies against the library's own velocity query with everything behind it restated in float32
(tests/velocity.py on tests/buoyancy.py) -- bit for bit, at every shape where the segmented reduction can go wrong --, against the pure
restatement on maps read back from the same frame, against ocean_buoyancy_bodies where the drag is off, and its readiness rules."""
import numpy as np
import pytest

import buoyancy as B
import velocity as V

pytestmark = pytest.mark.gpu
F = np.float32
GRID = 512
PHYS = dict(density=1025.0, gravity=9.81, drag=1000.0)
POINTS = [0, 1, 63, 64, 65, 130]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def random_hull(points, seed=0):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1.0, 1.0, (points, 3)) * [3.0, 0.75, 1.5], rng.uniform(0.2, 0.6, (points, 1))], axis=1).astype(np.float32)


class Sea:
    """`cascades` sources (tiles 0 ..) and their twins behind them, one frame, and the geometry every call of a test uses."""

    def __init__(self, n=64, cascades=1, lam=-1.0, seed=0x5EED, t=3.7):
        import watersurfacerendering_amd as W
        self.lengths = [1000.0, 370.0][:cascades]
        self.lam, self.cascades = lam, cascades
        self.b = W.OceanBatch(n, 2 * cascades, 0)
        for i, L in enumerate(self.lengths):
            self.b.set_params(tile=i, tile_length=L, lambda_=lam)
            self.b.set_velocity_twin(cascades + i, i)
        self.b.prepare(seed)
        self.b.compute_waves(t)
        self.scales = [1.0, 2.7][:cascades]
        self.vd = 1000.0 / GRID

    def geometry(self, k):
        return dict(first_tile=0, uv_scales=self.scales, grid_size=GRID, vertex_distance=self.vd, choppy=self.lam, iterations=k)

    def want(self, hull, bodies, k, **phys):
        """The definition with the library's own velocity query in the middle: world points formed on the host in the restated fp32 order,
        H, the residual and V from OceanBatch.query_velocity on the same frame, force, torque and tree finished in numpy."""
        bi, pi, hi = B.pairs(bodies, len(hull))
        _, p, _ = B.world_points(hull, bodies, bi, hi)
        pos, vel = self.b.query_velocity(np.stack([p[0], p[2]], axis=1), **self.geometry(k))
        return V.finish_flow(bodies, hull, bi, pi, hi, pos[:, 1], vel[:, 3], vel[:, :3], **dict(PHYS, **phys))[:2]

    def close(self):
        self.b.close()


def fleet_of(count, hull_points, seed):
    """count bodies whose point counts cycle through POINTS, each on its own stretch of the hull; moving and turning."""
    rng = np.random.default_rng(seed)
    counts = np.array([POINTS[(i + seed) % len(POINTS)] for i in range(count)], np.uint32)
    firsts = np.array([int(rng.integers(0, hull_points - c + 1)) for c in counts], np.uint32)
    return B.fleet(count, firsts, counts, seed=seed, half=600.0)


@pytest.mark.parametrize("cascades", [1, 2])
def test_every_output_is_the_velocity_query_behind_the_restated_sum(cascades):
    """Bodies 1, 4 and 5 (four per block), points per body 0, 1, 63, 64, 65 and 130, K = 1 and 8: np.array_equal on all eight outputs."""
    import torch
    sea = Sea(64, cascades)
    hull = random_hull(200, seed=cascades)
    sea.b.set_hull(hull)
    for k in (1, 8):
        for count in (1, 4, 5):
            for seed in range(len(POINTS)):                 # every body slot sees every point count
                fleet = fleet_of(count, len(hull), seed)
                force, torque = sea.b.buoyancy_flow(fleet, **sea.geometry(k))
                wf, wt = sea.want(hull, fleet, k)
                assert np.array_equal(bits(force), bits(wf)), (cascades, k, count, seed)
                assert np.array_equal(bits(torque), bits(wt)), (cascades, k, count, seed)
                for i in np.nonzero(fleet["points"] == 0)[0]:
                    assert not bits(force[i]).any() and not bits(torque[i]).any()
    # the device form, ranges that leave the hull clamped as in ocean_buoyancy_bodies_device
    fleet = np.concatenate([fleet_of(5, len(hull), 3), B.fleet(3, 150, 70, seed=9, half=300.0)])
    fleet["pos"][-3:, 1] = -100.0                           # far under the deepest trough: every cell that is summed counts whole
    d_bodies = torch.from_numpy(np.ascontiguousarray(fleet).view(np.int32).reshape(-1, 16)).cuda()
    d_force = torch.full((len(fleet), 4), float("nan"), dtype=torch.float32, device="cuda")
    d_torque = torch.full_like(d_force, float("nan"))
    torch.cuda.synchronize()
    sea.b.buoyancy_flow_device(d_bodies.data_ptr(), len(fleet), d_force.data_ptr(), d_torque.data_ptr(), **sea.geometry(8))
    sea.b.synchronize()
    wf, wt = sea.want(hull, fleet, 8)                       # (B.pairs clamps as the header says)
    assert np.array_equal(bits(d_force.cpu().numpy()), bits(wf)) and np.array_equal(bits(d_torque.cpu().numpy()), bits(wt))
    assert np.isfinite(wf).all()
    clamped = float((hull[150:, 3].astype(np.float64) ** 3).sum())      # 50 of the 70 points each of them asks for
    assert wf[-3:, 3] == pytest.approx([clamped] * 3, rel=1e-5)
    import watersurfacerendering_amd as W
    with pytest.raises(W.OceanError) as e:
        sea.b.buoyancy_flow(fleet, **sea.geometry(8))       # the host form sees the ranges and refuses
    assert e.value.code == W._abi.OCEAN_E_INVALID
    sea.close()


def test_without_drag_it_is_ocean_buoyancy_bodies_bit_for_bit():
    sea = Sea(64, 2)
    hull = random_hull(200, seed=5)
    sea.b.set_hull(hull)
    for count in (1, 4, 5):
        fleet = fleet_of(count, len(hull), count)
        flow = sea.b.buoyancy_flow(fleet, **sea.geometry(8), drag=0.0)
        still = sea.b.buoyancy(fleet, **sea.geometry(8), drag=0.0)
        assert np.array_equal(bits(flow[0]), bits(still[0])) and np.array_equal(bits(flow[1]), bits(still[1]))
    # with drag the two differ: the water moves
    fleet = fleet_of(5, len(hull), 1)
    fleet["pos"][:, 1] = -3.0
    assert not np.array_equal(bits(sea.b.buoyancy_flow(fleet, **sea.geometry(8))[0]), bits(sea.b.buoyancy(fleet, **sea.geometry(8))[0]))
    sea.close()


def test_a_body_at_rest_under_the_sea_is_pushed_the_way_the_water_goes():
    """One cell of 0.5 m per body, 100 m down (the heights of this sea reach tens of metres: fully submerged whatever the wave), at rest: F.x and F.z are drag * volume * V.x, V.z of the water
    at the cell, so they carry the sign of the local water velocity (bodies where that is under 0.05 m/s are left out)."""
    sea = Sea(64, 1)
    hull = np.array([[0.0, 0.0, 0.0, 0.5]], np.float32)
    sea.b.set_hull(hull)
    rng = np.random.default_rng(12)
    fleet = B.make_bodies(5 * 13)
    fleet["pos"] = np.stack([rng.uniform(-600, 600, len(fleet)), np.full(len(fleet), -100.0), rng.uniform(-600, 600, len(fleet))], axis=1)
    fleet["points"] = 1
    force, torque = sea.b.buoyancy_flow(fleet, **sea.geometry(8))
    _, vel = sea.b.query_velocity(np.ascontiguousarray(fleet["pos"][:, [0, 2]]), **sea.geometry(8))
    assert np.all(force[:, 3] == F(0.125))
    for axis in (0, 2):
        moving = np.abs(vel[:, axis]) > 0.05
        assert moving.sum() > len(fleet) // 4
        assert np.array_equal(np.sign(force[moving, axis]), np.sign(vel[moving, axis]))
        assert np.array_equal(bits(force[:, axis]), bits(F(0.0) + (-(F(1000.0) * F(0.125))) * (F(0.0) - vel[:, axis])))
    sea.close()


def test_kernel_matches_restatement():
    """The rule of tests/test_buoyancy_gpu.py: lambda = -0.5, K = 16, 300 bodies of 64 points, maps read back from the same frame.  A body all
    of whose points have a restatement residual < 1e-3 m agrees within 1e-5 of the sum of |term| in each of the eight channels; at most 1 %
    of the bodies may be left out."""
    sea = Sea(64, 1, lam=-0.5, seed=0x5EED0040)
    hull = B.box_hull(8, 2, 4, 0.5)
    sea.b.set_hull(hull)
    fleet = B.fleet(300, 0, 64, seed=65)
    force, torque = sea.b.buoyancy_flow(fleet, **sea.geometry(16))
    d, q = sea.b.read_maps()
    c = sea.cascades
    amps = [sea.b.heights(i)[0] for i in range(2 * c)]
    bi, pi, hi = B.pairs(fleet, len(hull))
    _, p, _ = B.world_points(hull, fleet, bi, hi)
    pos, vel = V.query_velocity(list(d[:c]), list(q[:c]), amps[:c], list(d[c:]), amps[c:], [sea.lam] * c, sea.lengths, sea.scales, GRID, sea.vd,
                                sea.lam, np.stack([p[0], p[2]], axis=1), 16)
    wf, wt, mag = V.finish_flow(fleet, hull, bi, pi, hi, pos[:, 1], vel[:, 3], vel[:, :3], **PHYS)
    worst = np.maximum.reduceat(vel[:, 3], np.arange(0, len(bi), 64))
    ok = worst < 1e-3
    got = np.concatenate([force[:, :3], torque[:, :3], force[:, 3:], torque[:, 3:]], axis=1).astype(np.float64)
    want = np.concatenate([wf[:, :3], wt[:, :3], wf[:, 3:], wt[:, 3:]], axis=1).astype(np.float64)
    err = np.abs(got - want) / np.maximum(mag, 1e-30)
    same = int(((bits(force) == bits(wf)).all(1) & (bits(torque) == bits(wt)).all(1)).sum())
    print(f"{same}/{len(fleet)} bodies bit-identical; {int((~ok).sum())} left out; largest error / sum|term| per channel "
          f"{dict(zip(B.CHANNELS, np.round(err[ok].max(0), 9)))}; wet {int((wf[:, 3] > 0).sum())}")
    assert (~ok).sum() <= 0.01 * len(fleet)
    assert (wf[:, 3] > 0).sum() > 60
    assert (err[ok] <= 1e-5).all(), np.nonzero((err > 1e-5).any(1) & ok)[0]
    sea.close()


def test_readiness_and_twin_errors():
    import watersurfacerendering_amd as W
    A = W._abi
    b = W.OceanBatch(16, 3, 0)
    b.prepare(3)
    b.compute_waves(1.0)
    fleet = B.fleet(4, 0, 10, seed=2)
    geo = dict(grid_size=GRID, vertex_distance=1000.0 / GRID)
    with pytest.raises(W.OceanError) as e:
        b.buoyancy_flow(fleet, **geo)
    assert e.value.code == A.OCEAN_E_NOT_READY                           # no hull (and no twin)
    b.set_hull(random_hull(20, seed=1))
    with pytest.raises(W.OceanError) as e:
        b.buoyancy_flow(fleet, **geo)
    assert e.value.code == A.OCEAN_E_NOT_READY                           # a hull, but no tile of the set has a twin
    b.buoyancy(fleet, **geo)                                             # (the still-water call does not need one)
    b.set_velocity_twin(2, 0)
    b.prepare(3)
    b.compute_waves(1.0)
    b.buoyancy_flow(fleet, **geo)
    for kw, code in ((dict(uv_scales=(1.0, 1.0)), A.OCEAN_E_INVALID),    # tile 0 has a twin, tile 1 has none
                     (dict(first_tile=1), A.OCEAN_E_NOT_READY), (dict(drag=-1.0), A.OCEAN_E_INVALID), (dict(iterations=33), A.OCEAN_E_INVALID)):
        with pytest.raises(W.OceanError) as e:
            b.buoyancy_flow(fleet, **dict(geo, **kw))
        assert e.value.code == code, kw
    b.close()
