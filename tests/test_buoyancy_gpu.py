"""Buoyancy on the MI355X (include/ocean_consumers.h: ocean_set_hull, ocean_buoyancy_bodies / _device): the HIP kernel against the library's
own surface query with everything behind the query restated in float32 (tests/buoyancy.py) -- bit for bit, at every shape where the
segmented reduction can go wrong --, against the pure restatement on maps read back from the same frame, and the API's device variant,
ordering, bound output, hull lifetime and error rules."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import buoyancy as B
import surface_raycast as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LENGTHS3 = [1000.0, 370.0, 93.0]        # the cascade set of tests/test_surface_query_gpu.py
F = np.float32
GRID = 512
PHYS = dict(density=1025.0, gravity=9.81, drag=1000.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def words(bodies):
    """[count, 16] int32: the records' bytes as a torch tensor can carry them."""
    return np.ascontiguousarray(bodies).view(np.int32).reshape(-1, 16)


def random_hull(points, seed=0):
    """Cells of 0.2 .. 0.6 m scattered through a 6 x 1.5 x 3 m box: no order a reduction could lean on."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(-1.0, 1.0, (points, 3)) * [3.0, 0.75, 1.5], rng.uniform(0.2, 0.6, (points, 1))], axis=1).astype(np.float32)


class Sea:
    """One context with a frame on it, the geometry every call of a test uses, and (on demand) the frame's maps as a restated surface."""

    def __init__(self, n=64, cascades=1, lam=-1.0, seed=0x5EED, t=3.7, **params):
        import watersurfacerendering_amd as W
        self.lengths = [1000.0] if cascades == 1 else LENGTHS3
        self.lam = lam
        self.b = W.OceanBatch(n, len(self.lengths), 0)
        for i, L in enumerate(self.lengths):
            self.b.set_params(tile=i, tile_length=L, lambda_=lam, **params)
        self.b.prepare(seed)
        self.amps = [float(a) for a in self.b.compute_waves(t)]
        self.scales = [self.lengths[0] / L for L in self.lengths]
        self.vd = self.lengths[0] / GRID

    def geometry(self, k):
        return dict(first_tile=0, uv_scales=self.scales, grid_size=GRID, vertex_distance=self.vd, choppy=self.lam, iterations=k)

    def restated(self, k):
        disp, nrm = self.b.read_maps()
        return R.Surface(list(disp), list(nrm), self.amps, [self.lam] * len(self.lengths), self.lengths, self.scales, GRID, self.vd, self.lam, k)

    def want(self, hull, bodies, k, **phys):
        """The definition with the library's own query in the middle: world points formed on the host in the restated fp32 order, H and res
        from OceanBatch.query_surface on the same frame, force, torque and tree finished in numpy."""
        bi, pi, hi = B.pairs(bodies, len(hull))
        _, p, _ = B.world_points(hull, bodies, bi, hi)
        pos, nrm = self.b.query_surface(np.stack([p[0], p[2]], axis=1), **self.geometry(k))
        return B.finish(bodies, hull, bi, pi, hi, pos[:, 1], nrm[:, 3], **dict(PHYS, **phys))[:2]

    def check_exact(self, hull, bodies, k, tag, **phys):
        force, torque = self.b.buoyancy(bodies, **self.geometry(k), **phys)
        wf, wt = self.want(hull, bodies, k, **phys)
        assert np.array_equal(bits(force), bits(wf)), (tag, np.nonzero((bits(force) != bits(wf)).any(1))[0][:8])
        assert np.array_equal(bits(torque), bits(wt)), (tag, np.nonzero((bits(torque) != bits(wt)).any(1))[0][:8])
        return force, torque

    def close(self):
        self.b.close()


POINTS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 200]


def mixed_fleet(hull_points, seed):
    """One body per entry of POINTS, each on its own stretch of the hull, then bodies that share one range, bodies whose ranges overlap,
    one far above the water and one far below it: 18 bodies."""
    rng = np.random.default_rng(seed)
    counts = POINTS + [37, 37, 37, 100, 100, 100, 64, 64]
    firsts = [int(rng.integers(0, hull_points - c + 1)) for c in POINTS] + [11, 11, 11, 50, 90, 130, 0, 0]
    b = B.fleet(len(counts), np.array(firsts, np.uint32), np.array(counts, np.uint32), seed=seed, half=600.0)
    b["pos"][-2, 1], b["pos"][-1, 1] = 100.0, -100.0
    return b


@pytest.mark.parametrize("cascades", [1, 3])
def test_every_output_is_the_query_behind_the_restated_sum(cascades):
    """Rough sea (lambda = -1), K = 1 and 8: np.array_equal on all eight outputs of every body.  Pins the transform, the force, the segment
    handling and the order of the reduction whatever Newton does.  Body counts 1, 3, 4, 5, 9 leave blocks partly filled; 18 covers the
    points per body 0 .. 200, shared and overlapping ranges, a body above the water (+0.0f in every sum) and one under it."""
    sea = Sea(64, cascades)
    hull = random_hull(230, seed=cascades)
    sea.b.set_hull(hull)
    fleet = mixed_fleet(len(hull), seed=10 + cascades)
    for k in (1, 8):
        force, torque = sea.check_exact(hull, fleet, k, (cascades, k, "mixed"))
        assert not bits(force[0]).any() and not bits(torque[0]).any()                    # no points
        assert not bits(force[-2]).any() and not bits(torque[-2, :3]).any()              # above the water, moving: every sum still +0.0f
        assert torque[-2, 3] > 0.0                                                       # (its residual is the query's, wet or dry: the header)
        assert force[-1, 3] == pytest.approx(float((hull[:64, 3].astype(np.float64) ** 3).sum()), rel=1e-5)     # under it: every cell whole
        assert (force[1:10, 3] > 0.0).sum() >= 3
        for count in (1, 3, 4, 5, 9):
            sub = np.roll(fleet, -count)[:count]
            sea.check_exact(hull, sub, k, (cascades, k, count))
    # bodies that share a range AND a pose are the same body: the same bits, wherever they sit in the call
    twins = np.repeat(fleet[12:13], 7)
    force, torque = sea.check_exact(hull, twins, 8, (cascades, "twins"))
    assert (bits(force) == bits(force[0])).all() and (bits(torque) == bits(torque[0])).all()
    sea.close()


def test_a_flat_sea_is_the_pure_restatement_bit_for_bit():
    """phillips_const = 0: every height is 0 and Newton has nothing to do, so the kernel and numpy agree without the query in between."""
    sea = Sea(64, 1, phillips_const=0.0)
    hull = np.concatenate([B.box_hull(4, 4, 4, 0.25), random_hull(170, seed=5)])
    sea.b.set_hull(hull)
    fleet = mixed_fleet(len(hull), seed=20)
    fleet["first_point"][-1], fleet["pos"][-1], fleet["quat"][-1] = 0, (3.0, 0.0, -2.0), (0.0, 0.0, 0.0, 1.0)
    fleet["vel"][-1], fleet["omega"][-1] = 0.0, 0.0
    force, torque = sea.b.buoyancy(fleet, **sea.geometry(8))
    wf, wt, _ = B.buoyancy(sea.restated(8), hull, fleet, **PHYS)
    assert np.array_equal(bits(force), bits(wf)) and np.array_equal(bits(torque), bits(wt))
    assert force[-1, 3] == F(0.5) and force[-1, 1] == F(1025.0) * F(9.81) * F(0.5)       # the binary box: half its volume, exactly
    assert np.all(torque[:, 3] == 0.0)
    assert not bits(force[-2]).any() and not bits(torque[-2]).any()                      # above a flat sea: +0.0f in all eight outputs
    sea.close()


@pytest.mark.parametrize("n,cascades", [(64, 1), (64, 3), (256, 1), (256, 3)])
def test_kernel_matches_restatement(n, cascades):
    """lambda = -0.5, K = 16 (tests/test_buoyancy.py shows that this setting leaves every residual under 1e-3 m), 300 bodies of 64 points,
    maps read back from the same frame.  A body all of whose points have a restatement residual < 1e-3 m agrees within 1e-5 of the sum of
    |term| in each of the eight channels, the largest residual against the sum of its points' residuals among them -- the project's 1e-5
    parity bound carried through a sum.  At most 1 % of the bodies may be left out."""
    sea = Sea(n, cascades, lam=-0.5, seed=0x5EED0000 + n)
    hull = B.box_hull(8, 2, 4, 0.5)
    sea.b.set_hull(hull)
    fleet = B.fleet(300, 0, 64, seed=n + cascades)
    force, torque = sea.b.buoyancy(fleet, **sea.geometry(16))
    wf, wt, mag, bi, res = B.buoyancy(sea.restated(16), hull, fleet, detail=True, **PHYS)
    worst = np.maximum.reduceat(res, np.arange(0, len(res), 64))
    ok = worst < 1e-3
    got = np.concatenate([force[:, :3], torque[:, :3], force[:, 3:], torque[:, 3:]], axis=1).astype(np.float64)
    want = np.concatenate([wf[:, :3], wt[:, :3], wf[:, 3:], wt[:, 3:]], axis=1).astype(np.float64)
    err = np.abs(got - want) / np.maximum(mag, 1e-30)
    same = int(((bits(force) == bits(wf)).all(1) & (bits(torque) == bits(wt)).all(1)).sum())
    print(f"n={n} cascades={cascades}: {same}/{len(fleet)} bodies bit-identical; {int((~ok).sum())} left out; "
          f"largest error / sum|term| per channel {dict(zip(B.CHANNELS, np.round(err[ok].max(0), 9)))}; wet {int((wf[:, 3] > 0).sum())}")
    assert (~ok).sum() <= 0.01 * len(fleet)
    assert (wf[:, 3] > 0).sum() > 60
    assert (err[ok] <= 1e-5).all(), np.nonzero((err > 1e-5).any(1) & ok)[0]
    sea.close()


def test_device_variant_is_bit_identical_to_the_host_call():
    import torch
    sea = Sea(64, 3)
    hull = random_hull(230, seed=3)
    sea.b.set_hull(hull)
    fleet = np.concatenate([mixed_fleet(len(hull), 30), B.fleet(1000, 20, 70, seed=31)])
    force, torque = sea.b.buoyancy(fleet, **sea.geometry(8))
    d_bodies = torch.from_numpy(words(fleet)).cuda()
    d_force = torch.full((len(fleet), 4), float("nan"), dtype=torch.float32, device="cuda")
    d_torque = torch.full_like(d_force, float("nan"))
    torch.cuda.synchronize()
    sea.b.buoyancy_device(d_bodies.data_ptr(), len(fleet), d_force.data_ptr(), d_torque.data_ptr(), **sea.geometry(8))
    sea.b.synchronize()
    assert np.array_equal(bits(d_force.cpu().numpy()), bits(force)) and np.array_equal(bits(d_torque.cpu().numpy()), bits(torque))
    sea.close()


def test_device_form_clamps_a_range_that_leaves_the_hull():
    """Where the host cannot see the bodies the kernel clamps: points past the end are not summed, a first_point past the end sums none.
    The library keeps a guard of NaN points behind the hull, so a body that read past the end would not come out finite -- and the
    result is the clamped definition, with the library's own query in the middle, bit for bit."""
    import torch
    import watersurfacerendering_amd as W
    sea = Sea(64, 1)
    hull = random_hull(100, seed=4)
    sea.b.set_hull(hull)
    fleet = B.fleet(6, 0, 0, seed=40, half=300.0)
    fleet["pos"][:, 1] = -8.0                                        # well under the water: every cell that is summed counts
    fleet["first_point"], fleet["points"] = [90, 0, 99, 100, 4000000000, 37], [11, 0xFFFFFFFF, 2, 1, 4000000000, 64]
    with pytest.raises(W.OceanError) as e:
        sea.b.buoyancy(fleet, **sea.geometry(8))                     # the host form sees them and refuses before any launch
    assert e.value.code == W._abi.OCEAN_E_INVALID
    d_bodies = torch.from_numpy(words(fleet)).cuda()
    d_force = torch.full((len(fleet), 4), float("nan"), dtype=torch.float32, device="cuda")
    d_torque = torch.full_like(d_force, float("nan"))
    torch.cuda.synchronize()
    sea.b.buoyancy_device(d_bodies.data_ptr(), len(fleet), d_force.data_ptr(), d_torque.data_ptr(), **sea.geometry(8))
    sea.b.synchronize()
    force, torque = d_force.cpu().numpy(), d_torque.cpu().numpy()
    wf, wt = sea.want(hull, fleet, 8)                                # (B.pairs clamps as the header says)
    assert np.isfinite(force).all() and np.isfinite(torque).all()
    assert np.array_equal(bits(force), bits(wf)) and np.array_equal(bits(torque), bits(wt))
    assert force[0, 3] > 0.0 and force[1, 3] > force[0, 3] and not bits(force[3]).any() and not bits(force[4]).any()
    sea.close()


def test_pipelined_context_answers_for_its_most_recent_frame_among_other_consumers():
    import torch
    import watersurfacerendering_amd as W
    hull = random_hull(130, seed=6)
    fleet = B.fleet(500, 0, 130, seed=60)
    geo = dict(grid_size=GRID, vertex_distance=1000.0 / GRID)
    s = W.OceanBatch(64, 1, 0)
    s.prepare(9)
    s.compute_waves(2.5)
    s.set_hull(hull)
    want = s.buoyancy(fleet, **geo)
    s.close()
    p = W.OceanBatch(64, 1, 0)
    p.set_pipeline_depth(3)
    p.set_hull(hull)
    p.prepare(9)
    xz = torch.from_numpy(np.ascontiguousarray(fleet["pos"][:, [0, 2]])).cuda()
    d_bodies = torch.from_numpy(words(fleet)).cuda()
    out = [torch.zeros((len(fleet), 4), dtype=torch.float32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    for t in (0.5, 1.5, 2.5):                                          # three chains, three streams; every consumer between the frames
        p.compute_waves_async(t)
        p.update_foam(0.1)
        p.query_surface_device(xz.data_ptr(), len(fleet), out[0].data_ptr(), out[1].data_ptr(), **geo)
        p.buoyancy_device(d_bodies.data_ptr(), len(fleet), out[2].data_ptr(), out[3].data_ptr(), **geo)
        W._abi.check(p._L.ocean_build_mips(p._h, 0), "ocean_build_mips")
    got = p.buoyancy(fleet, **geo)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    p.synchronize()
    assert np.array_equal(bits(out[2].cpu().numpy()), bits(want[0])) and np.array_equal(bits(out[3].cpu().numpy()), bits(want[1]))
    p.close()


def test_buoyancy_reads_caller_bound_maps():
    import torch
    import watersurfacerendering_amd as W
    n = 64
    hull = B.box_hull(4, 4, 4, 0.25)
    fleet = B.fleet(64, 0, 64, seed=7)
    ref = W.OceanBatch(n, 1, 0)
    ref.prepare(21)
    ref.compute_waves(3.7)
    ref.set_hull(hull)
    want = ref.buoyancy(fleet)
    ref.close()
    maps = torch.zeros((2, n, n, 4), dtype=torch.float32, device="cuda")
    b = W.OceanBatch(n, 1, 0)
    b.bind_output(maps[0].data_ptr(), maps[1].data_ptr())
    b.prepare(21)
    b.compute_waves(3.7)
    b.set_hull(hull)
    got = b.buoyancy(fleet)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    b.synchronize()
    maps.zero_()                        # the call reads the bound memory where it is: flat water at height 0 from now on
    torch.cuda.synchronize()
    level = B.make_bodies(2)
    level["pos"], level["points"] = [(3.0, 0.0, -2.0), (8.0, -9.0, 1.0)], 64
    force, torque = b.buoyancy(level, drag=0.0)
    w = F(1025.0) * F(9.81)
    assert np.array_equal(force, np.array([[0.0, w * F(0.5), 0.0, 0.5], [0.0, w, 0.0, 1.0]], np.float32)) and not torque.any()
    b.bind_output(None, None)
    b.close()


def test_the_hull_outlives_the_maps_and_can_be_replaced():
    import watersurfacerendering_amd as W
    A = W._abi
    hull_a, hull_b = random_hull(100, seed=8), random_hull(37, seed=9)
    fleet = B.fleet(40, 0, 37, seed=80)

    def fresh(n, hull):
        r = W.OceanBatch(n, 1, 0)
        r.prepare(5)
        r.compute_waves(1.25)
        r.set_hull(hull)
        out = r.buoyancy(fleet)
        r.close()
        return out

    b = W.OceanBatch(64, 1, 0)
    b.set_hull(hull_a)                                                 # before anything is prepared: the hull does not need the maps
    with pytest.raises(W.OceanError) as e:
        b.buoyancy(fleet)
    assert e.value.code == A.OCEAN_E_NOT_READY                         # ... but the call needs a frame
    b.prepare(5)
    with pytest.raises(W.OceanError) as e:
        b.buoyancy(fleet)
    assert e.value.code == A.OCEAN_E_NOT_READY
    b.compute_waves(1.25)
    want = fresh(64, hull_a)
    got = b.buoyancy(fleet)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    b.prepare(5)                                                       # a new Prepare keeps the hull
    b.compute_waves(1.25)
    got = b.buoyancy(fleet)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    b.set_tile_size(128)                                               # ... and so does a new tile size
    b.prepare(5)
    b.compute_waves(1.25)
    want = fresh(128, hull_a)
    got = b.buoyancy(fleet)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    b.set_hull(hull_b)                                                 # replaced between two calls
    want = fresh(128, hull_b)
    got = b.buoyancy(fleet)
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    for bad in ((0, 3, 0.0), (1, 3, -0.5), (2, 3, np.inf), (3, 3, np.nan), (4, 0, np.nan), (36, 2, np.inf)):
        h = hull_a.copy()
        h[bad[0], bad[1]] = bad[2]
        with pytest.raises(W.OceanError) as e:
            b.set_hull(h)
        assert e.value.code == A.OCEAN_E_INVALID, bad
    got = b.buoyancy(fleet)                                            # a refused hull leaves the old one
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
    b.set_hull(None)                                                   # dropped
    with pytest.raises(W.OceanError) as e:
        b.buoyancy(fleet)
    assert e.value.code == A.OCEAN_E_NOT_READY
    b.close()


def test_argument_errors():
    import watersurfacerendering_amd as W
    A = W._abi
    b = W.OceanBatch(64, 2, 0)
    b.prepare(3)
    b.compute_waves(1.0)
    hull = random_hull(50, seed=1)
    fleet = B.fleet(8, 10, 40, seed=2)
    L, s, p = b._L, b._surface(0, (1.0,), None, None, -1.0, 8), b.buoyancy_params()
    words = W.OceanBatch._body_words(fleet)
    ptr = words.ctypes.data_as(C.c_void_p)
    out = np.zeros((2, 8, 4), np.float32)
    o0, o1 = out[0].ctypes.data_as(C.c_void_p), out[1].ctypes.data_as(C.c_void_p)
    assert L.ocean_buoyancy_bodies(b._h, C.byref(s), C.byref(p), ptr, 8, o0, o1) == A.OCEAN_E_NOT_READY          # no hull yet
    assert L.ocean_buoyancy_bodies_device(b._h, C.byref(s), C.byref(p), None, 0, None, None) == A.OCEAN_E_NOT_READY
    assert L.ocean_set_hull(b._h, None, 3) == A.OCEAN_E_INVALID
    b.set_hull(hull)
    for kw in (dict(uv_scales=(1.0,) * 3), dict(first_tile=2), dict(grid_size=0), dict(iterations=33), dict(density=-1.0),
               dict(gravity=float("nan")), dict(drag=float("inf")), dict(drag=-1e-3)):
        with pytest.raises(W.OceanError) as e:
            b.buoyancy(fleet, **kw)
        assert e.value.code == A.OCEAN_E_INVALID, kw
    for first, points in ((11, 40), (50, 1), (0xFFFFFFFF, 2), (3, 0xFFFFFFFF)):       # (the last two: the sum does not wrap)
        bad = fleet.copy()
        bad["first_point"][5], bad["points"][5] = first, points
        with pytest.raises(W.OceanError) as e:
            b.buoyancy(bad)
        assert e.value.code == A.OCEAN_E_INVALID, (first, points)
    edge = fleet.copy()
    edge["first_point"][5], edge["points"][5] = 50, 0                                   # an empty range at the end is inside
    assert not bits(b.buoyancy(edge)[0][5]).any()
    assert L.ocean_buoyancy_bodies(b._h, None, C.byref(p), ptr, 8, o0, o1) == A.OCEAN_E_INVALID
    assert L.ocean_buoyancy_bodies(b._h, C.byref(s), None, ptr, 8, o0, o1) == A.OCEAN_E_INVALID
    assert L.ocean_buoyancy_bodies(b._h, C.byref(s), C.byref(p), None, 8, o0, o1) == A.OCEAN_E_INVALID
    assert L.ocean_buoyancy_bodies(b._h, C.byref(s), C.byref(p), ptr, 8, None, o1) == A.OCEAN_E_INVALID
    assert L.ocean_buoyancy_bodies(b._h, C.byref(s), C.byref(p), ptr, 8, o0, None) == A.OCEAN_E_INVALID
    assert L.ocean_buoyancy_bodies_device(b._h, C.byref(s), C.byref(p), None, 8, None, None) == A.OCEAN_E_INVALID
    assert L.ocean_buoyancy_bodies(b._h, C.byref(s), C.byref(p), None, 0, None, None) == A.OCEAN_OK              # count = 0: nothing to do
    assert L.ocean_buoyancy_bodies_device(b._h, C.byref(s), C.byref(p), None, 0, None, None) == A.OCEAN_OK
    force, torque = b.buoyancy(fleet, first_tile=1, iterations=32, density=1000.0, gravity=1.62, drag=0.0)
    assert force.shape == (8, 4) and np.isfinite(force).all() and np.all(force[:, [0, 2]] == 0.0)
    b.close()


def test_cpp_adaptor_buoyancy_matches_python_binding(tmp_path):
    import watersurfacerendering_amd as W
    from watersurfacerendering_amd import _abi
    exe = tmp_path / "buoyancy_demo"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "buoyancy_demo.cpp"), "-o", str(exe),
                    "-L", os.path.dirname(_abi.LIB_PATH), "-locean_hip", "-Wl,-rpath," + os.path.dirname(_abi.LIB_PATH),
                    "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = tmp_path / "buoyancy.bin"
    r = subprocess.run([str(exe), "128", str(out), "3.7"], capture_output=True, text=True, check=True)
    n, amp, count, afloat = r.stdout.split()
    count, points = int(count), 36
    raw = np.fromfile(out, dtype=np.float32)
    hull = raw[:4 * points].reshape(points, 4)
    bodies = raw[4 * points:4 * points + 16 * count].view(B.BODY_DTYPE)
    cforce = raw[4 * points + 16 * count:4 * points + 20 * count].reshape(count, 4)
    ctorque = raw[4 * points + 20 * count:].reshape(count, 4)
    assert len(bodies) == count == 225 and np.all(bodies["points"] == points)
    ws = W.WSTessendorf(128, 1000.0)
    ws.SetWindDirection((1.0, 0.5)); ws.SetWindSpeed(20.0); ws.SetLambda(-1.5)
    ws.Prepare(seed=42)
    assert ws.ComputeWaves(3.7) == pytest.approx(float(amp), rel=1e-7)
    ws.SetHull(hull)
    force, torque = ws.Buoyancy(bodies)
    assert np.array_equal(bits(force), bits(cforce)) and np.array_equal(bits(torque), bits(ctorque))
    assert int(afloat) == int((force[:, 3] > 0).sum()) > count // 4
