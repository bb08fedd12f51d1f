"""Ray cast on the MI355X (include/ocean_consumers.h: ocean_raycast_surface / ocean_raycast_surface_device): the HIP kernel against the
float32 restatement (tests/surface_raycast.py) on maps read back from the same frame, its hits against the surface query, and the API's
device variant, ordering, bound output, size and error rules."""
import os
import subprocess

import numpy as np
import pytest

import surface_raycast as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LENGTHS3 = [1000.0, 370.0, 93.0]        # the cascade set of tests/test_surface_query_gpu.py
F = np.float32


def _rays(kind, count, hmax, seed=0):
    """camera: a frustum of rays from one eye 2..30 m above the slab, 5..60 degrees below the horizon (most hit, some graze);
    random: origins over +-600 m from under the water to 40 m above the slab, any direction (hits, misses and origins under water)."""
    rng = np.random.default_rng(seed)
    if kind == "camera":
        side = int(np.sqrt(count))
        eye = np.array([rng.uniform(-100, 100), hmax + rng.uniform(2.0, 30.0), rng.uniform(-100, 100)], np.float32)
        yaw = np.linspace(-0.8, 0.8, side) + rng.uniform(0, 2 * np.pi)
        pitch = np.linspace(np.radians(5.0), np.radians(60.0), side)
        yy, pp = np.meshgrid(yaw, pitch)
        d = np.stack([np.cos(pp) * np.sin(yy), -np.sin(pp), np.cos(pp) * np.cos(yy)], axis=-1).reshape(-1, 3)
        o = np.broadcast_to(eye, d.shape)
    else:
        o = np.stack([rng.uniform(-600, 600, count), rng.uniform(-hmax - 2.0, hmax + 40.0, count), rng.uniform(-600, 600, count)], 1)
        d = rng.normal(size=(count, 3))
        d[:, 1] -= 0.6                                                      # mostly downwards
    return np.concatenate([o, d], axis=1).astype(np.float32)


def _batch_with_maps(n, lengths, seed, t=3.7):
    import watersurfacerendering_amd as W
    b = W.OceanBatch(n, len(lengths), 0)
    for i, L in enumerate(lengths):
        b.set_params(tile=i, tile_length=L)
    b.prepare(seed)
    amps = [float(a) for a in b.compute_waves(t)]
    disp, nrm = b.read_maps()
    return b, amps, disp, nrm


def _compare(hit, nrm, ohit, onrm, closest, tag):
    """Every ray's status agrees; >= 99.9 % of rays are bit-identical, and every other one is a near-tie (the restatement's |f| came
    within 1e-4 m of zero at a deciding sample).  Returns the number of bit-identical rays."""
    status = lambda h: np.where(h[:, 3] >= 0.0, 0, np.where(h[:, 3] == -2.0, 2, 1))
    assert np.array_equal(status(hit), status(ohit)), (tag, int((status(hit) != status(ohit)).sum()))
    same = np.all(np.concatenate([hit, nrm], 1).view(np.uint32) == np.concatenate([ohit, onrm], 1).view(np.uint32), axis=1)
    assert same.mean() >= 0.999, (tag, int((~same).sum()))
    assert np.all(closest[~same] < 1e-4), (tag, closest[~same])
    return int(same.sum())


@pytest.mark.parametrize("n,cascades", [(64, 1), (64, 3), (512, 1), (512, 3), (2048, 1), (2048, 3)])
def test_kernel_matches_restatement(n, cascades):
    lengths = [1000.0] if cascades == 1 else LENGTHS3
    b, amps, disp, nrm = _batch_with_maps(n, lengths, 0x5EED0000 + n)
    grid = 512
    vd = lengths[0] / grid
    scales = [lengths[0] / L for L in lengths]
    for k in (1, 8):
        surf = R.Surface(list(disp), list(nrm), amps, [-1.0] * len(lengths), lengths, scales, grid, vd, -1.0, k)
        for kind in ("camera", "random"):
            rays = _rays(kind, 1024 if n == 2048 else 4096, float(surf.hmax), seed=n + k)
            hit, nr = b.raycast_surface(rays[:, :3], rays[:, 3:], 1500.0, 0, 0, 0, scales, grid, vd, -1.0, k)
            ohit, onr, closest = R.raycast_surface(surf, rays, 1500.0, detail=True)
            same = _compare(hit, nr, ohit, onr, closest, (n, cascades, kind, k))
            counts = [int((hit[:, 3] >= 0).sum()), int((hit[:, 3] == -1).sum()), int((hit[:, 3] == -2).sum())]
            print(f"n={n} cascades={cascades} {kind} K={k}: {same}/{len(rays)} rays bit-identical; hit/miss/under {counts}")
    b.close()


@pytest.mark.parametrize("cascades", [1, 3])
def test_hits_are_the_query_at_the_hit_point(cascades):
    """Every hit's position and normal are ocean_query_surface at (p(t).x, p(t).z), p(t) formed on the host in the kernel's fp32 order;
    every origin under water is the query at (o.x, o.z)."""
    lengths = [1000.0] if cascades == 1 else LENGTHS3
    b, amps, _, _ = _batch_with_maps(256, lengths, 77)
    scales = [lengths[0] / L for L in lengths]
    grid, vd = 512, lengths[0] / 512
    hmax = F(1.001) * F(np.sum(np.asarray(amps, np.float32), dtype=np.float32))
    rays = np.concatenate([_rays("camera", 4096, float(hmax), 1), _rays("random", 8192, float(hmax), 2)])
    hit, nr = b.raycast_surface(rays[:, :3], rays[:, 3:], 1500.0, 0, 0, 0, scales, grid, vd, -1.0, 8)
    o, d, _ = R.unit_rays(rays)
    sel = hit[:, 3] >= 0.0
    t = hit[sel, 3]
    assert sel.sum() > 4000
    pos, qn = b.query_surface(np.stack([o[sel, 0] + t * d[sel, 0], o[sel, 2] + t * d[sel, 2]], 1), 0, scales, grid, vd, -1.0, 8)
    assert np.array_equal(hit[sel, :3], pos[:, :3]) and np.array_equal(nr[sel, :3], qn[:, :3])
    assert np.array_equal(nr[sel, 3], (o[sel, 1] + t * d[sel, 1]) - pos[:, 1])
    assert np.abs(nr[sel, 3]).max() < 1e-3
    under = hit[:, 3] == -2.0
    assert under.sum() > 100
    pos, qn = b.query_surface(o[under][:, [0, 2]], 0, scales, grid, vd, -1.0, 8)
    assert np.array_equal(hit[under, :3], pos[:, :3]) and np.array_equal(nr[under, 3], o[under, 1] - pos[:, 1])
    b.close()


def _batch(n=256, tiles=1, seed=5, t=3.7):
    import watersurfacerendering_amd as W
    b = W.OceanBatch(n, tiles, 0)
    b.prepare(seed)
    b.compute_waves(t)
    return b


def test_device_variant_is_bit_identical_to_the_host_call():
    import torch
    b = _batch()
    rays = _rays("random", 100000, 10.0, 3)
    hit, nr = b.raycast_surface(rays[:, :3], rays[:, 3:], 800.0, steps=128, refine=4)
    d_rays = torch.from_numpy(rays).cuda()
    d_hit = torch.empty((len(rays), 4), dtype=torch.float32, device="cuda")
    d_nrm = torch.empty_like(d_hit)
    torch.cuda.synchronize()
    b.raycast_surface_device(d_rays.data_ptr(), len(rays), d_hit.data_ptr(), d_nrm.data_ptr(), 800.0, steps=128, refine=4)
    b.synchronize()
    assert np.array_equal(d_hit.cpu().numpy(), hit) and np.array_equal(d_nrm.cpu().numpy(), nr)
    b.close()


def test_pipelined_context_answers_for_its_most_recent_frame():
    import watersurfacerendering_amd as W
    rays = _rays("random", 20000, 10.0, 4)
    s = _batch(512, seed=9, t=2.5)
    want = s.raycast_surface(rays[:, :3], rays[:, 3:], 1000.0)
    s.close()
    p = W.OceanBatch(512, 1, 0)
    p.set_pipeline_depth(3)
    p.prepare(9)
    for t in (0.5, 1.5, 2.5):
        p.compute_waves_async(t)
    got = p.raycast_surface(rays[:, :3], rays[:, 3:], 1000.0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    p.close()


def test_raycast_reads_caller_bound_maps():
    import torch
    import watersurfacerendering_amd as W
    n = 128
    rays = _rays("camera", 4096, 10.0, 5)
    ref = _batch(n, seed=21)
    want = ref.raycast_surface(rays[:, :3], rays[:, 3:], 1000.0)
    ref.close()
    maps = torch.zeros((2, n, n, 4), dtype=torch.float32, device="cuda")
    b = W.OceanBatch(n, 1, 0)
    b.bind_output(maps[0].data_ptr(), maps[1].data_ptr())
    b.prepare(21)
    b.compute_waves(3.7)
    got = b.raycast_surface(rays[:, :3], rays[:, 3:], 1000.0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    b.synchronize()
    maps.zero_()                        # the ray cast reads the bound memory where it is: flat water at height 0 from now on
    torch.cuda.synchronize()
    hit, nr = b.raycast_surface(rays[:, :3], rays[:, 3:], 1000.0)
    o, d, _ = R.unit_rays(rays)
    sel = hit[:, 3] >= 0.0
    assert sel.mean() > 0.9 and np.all(hit[sel, 1] == 0.0)
    assert np.abs(hit[sel, 3] - o[sel, 1] / -d[sel, 1]).max() <= 1e-3 * np.abs(hit[sel, 3]).max()
    assert np.all(nr[sel, :3] == np.array([0.0, 1.0, 0.0], np.float32))
    b.bind_output(None, None)
    b.close()


def test_a_million_rays_in_one_call():
    b, amps, disp, nrm = _batch_with_maps(2048, [1000.0], 6)
    surf = R.Surface(list(disp), list(nrm), amps, [-1.0], [1000.0], [1.0], 512, 1000.0 / 512, -1.0)
    count = 1 << 20
    rays = _rays("random", count, float(surf.hmax), 6)
    hit, nr = b.raycast_surface(rays[:, :3], rays[:, 3:], 1500.0, grid_size=512, vertex_distance=1000.0 / 512)
    assert hit.shape == (count, 4) and np.isfinite(hit).all() and np.isfinite(nr).all()
    idx = np.random.default_rng(0).choice(count, 4096, replace=False)
    idx.sort()
    ohit, onr, closest = R.raycast_surface(surf, rays[idx], 1500.0, detail=True)
    _compare(hit[idx], nr[idx], ohit, onr, closest, "2^20 rays")
    b.close()


def test_argument_and_readiness_errors():
    import ctypes as C
    import watersurfacerendering_amd as W
    A = W._abi
    b = W.OceanBatch(64, 2, 0)
    rays = _rays("random", 16, 5.0)
    o, d = rays[:, :3], rays[:, 3:]
    with pytest.raises(W.OceanError) as e:
        b.raycast_surface(o, d, 100.0)                              # nothing prepared
    assert e.value.code == A.OCEAN_E_NOT_READY
    b.prepare(3)
    with pytest.raises(W.OceanError) as e:
        b.raycast_surface(o, d, 100.0)                              # no frame yet
    assert e.value.code == A.OCEAN_E_NOT_READY
    b.compute_waves(1.0)
    for md, kw in ((100.0, dict(uv_scales=(1.0,) * 3)), (100.0, dict(first_tile=2)), (100.0, dict(grid_size=0)),
                   (100.0, dict(iterations=33)), (0.0, {}), (-1.0, {}), (float("inf"), {}), (float("nan"), {}),
                   (100.0, dict(steps=4097)), (100.0, dict(refine=9))):
        with pytest.raises(W.OceanError) as e:
            b.raycast_surface(o, d, md, **kw)
        assert e.value.code == A.OCEAN_E_INVALID, (md, kw)
    L, s, r = b._L, b._surface(0, (1.0,), None, None, -1.0, 8), b._raycast(100.0, 0, 0)
    assert L.ocean_raycast_surface(b._h, None, C.byref(r), None, 0, None, None) == A.OCEAN_E_INVALID
    assert L.ocean_raycast_surface(b._h, C.byref(s), None, None, 0, None, None) == A.OCEAN_E_INVALID
    assert L.ocean_raycast_surface(b._h, C.byref(s), C.byref(r), None, 4, None, None) == A.OCEAN_E_INVALID
    assert L.ocean_raycast_surface_device(b._h, C.byref(s), C.byref(r), None, 4, None, None) == A.OCEAN_E_INVALID
    assert L.ocean_raycast_surface(b._h, C.byref(s), C.byref(r), None, 0, None, None) == A.OCEAN_OK      # count = 0: nothing to do
    assert L.ocean_raycast_surface_device(b._h, C.byref(s), C.byref(r), None, 0, None, None) == A.OCEAN_OK
    hit, _ = b.raycast_surface(o, d, 100.0, steps=4096, refine=8, first_tile=1)
    assert hit.shape == (16, 4)
    b.close()


def test_a_later_lambda_does_not_change_the_hits():
    b = _batch(256, seed=8)
    rays = _rays("camera", 10000, 10.0, 7)
    want = b.raycast_surface(rays[:, :3], rays[:, 3:], 1000.0)
    b.set_lambda(-2.0)
    got = b.raycast_surface(rays[:, :3], rays[:, 3:], 1000.0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    b.compute_waves(3.7)                                            # a frame with the new lambda: a different surface
    assert not np.array_equal(b.raycast_surface(rays[:, :3], rays[:, 3:], 1000.0)[0], want[0])
    b.close()


def test_cpp_adaptor_raycast_matches_python_binding(tmp_path):
    import watersurfacerendering_amd as W
    from watersurfacerendering_amd import _abi
    exe = tmp_path / "raycast_demo"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "raycast_demo.cpp"), "-o", str(exe),
                    "-L", os.path.dirname(_abi.LIB_PATH), "-locean_hip", "-Wl,-rpath," + os.path.dirname(_abi.LIB_PATH),
                    "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = tmp_path / "raycast.bin"
    r = subprocess.run([str(exe), "128", str(out), "3.7"], capture_output=True, text=True, check=True)
    n, amp, count, hits = r.stdout.split()
    count = int(count)
    raw = np.fromfile(out, dtype=np.float32)
    o = raw[:3 * count].reshape(count, 3)
    d = raw[3 * count:6 * count].reshape(count, 3)
    chit = raw[6 * count:10 * count].reshape(count, 4)
    cnrm = raw[10 * count:].reshape(count, 4)
    ws = W.WSTessendorf(128, 1000.0)
    ws.SetWindDirection((1.0, 0.5)); ws.SetWindSpeed(20.0); ws.SetLambda(-1.5)
    ws.Prepare(seed=42)
    assert ws.ComputeWaves(3.7) == pytest.approx(float(amp), rel=1e-7)
    hit, nrm = ws.RaycastSurface(o, d, 500.0)
    assert np.array_equal(hit, chit) and np.array_equal(nrm, cnrm)
    assert int(hits) == int((hit[:, 3] >= 0).sum()) > count // 2
