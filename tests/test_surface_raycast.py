"""Ray cast (include/ocean_consumers.h: ocean_raycast_surface) on the CPU: properties of the float32 restatement (tests/surface_raycast.py)
on oracle maps -- vertical rays, oblique rays, a brute-force march, misses and origins under water -- the C ABI's argument checks without
a device, and the C++ adaptor's RaycastSurface compiling and linking.  The kernel against the restatement on the GPU:
tests/test_surface_raycast_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import surface_raycast as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS3 = [1000.0, 370.0, 93.0]
F = np.float32


def oracle_maps(n, seed=7, t=3.7, lam=-1.0, length=1000.0):
    from oracle import oracle as O
    prep = O.numpy_prepare(n, O.gauss_xi_numpy(seed, n), length=length)
    amp, d, q, _, _ = O.numpy_compute_waves(prep, t, lam=lam)
    return float(np.float32(amp)), d.astype(np.float32), q.astype(np.float32)


def surface(cascades, n=64, grid=256):
    """The default ocean (one 1000 m tile) or three tiles of one ocean as cascades, each keeping its metres per texel."""
    lengths = [1000.0] if cascades == 1 else LENGTHS3
    maps = [oracle_maps(n, seed=7 + i, length=L) for i, L in enumerate(lengths)]
    scales = [lengths[0] / L for L in lengths]
    return R.Surface([m[1] for m in maps], [m[2] for m in maps], [m[0] for m in maps], [-1.0] * len(lengths), lengths, scales,
                     grid, lengths[0] / grid, -1.0)


def oblique_rays(count, surf, seed=0, height=(1.0, 40.0)):
    """Origins above the slab or inside it (above the water), directions 5..80 degrees below the horizon, any heading."""
    rng = np.random.default_rng(seed)
    xz = rng.uniform(-400.0, 400.0, (count, 2)).astype(np.float32)
    y = (surf.hmax + rng.uniform(*height, count)).astype(np.float32)
    pitch = rng.uniform(np.radians(5.0), np.radians(80.0), count)
    yaw = rng.uniform(0.0, 2.0 * np.pi, count)
    d = np.stack([np.cos(pitch) * np.sin(yaw), -np.sin(pitch), np.cos(pitch) * np.cos(yaw)], axis=1) * rng.uniform(0.5, 3.0, (count, 1))
    return np.concatenate([xz[:, :1], y[:, None], xz[:, 1:], d], axis=1).astype(np.float32)


@pytest.mark.parametrize("cascades", [1, 3])
def test_vertical_rays_hit_the_queried_height(cascades):
    surf = surface(cascades)
    rng = np.random.default_rng(1)
    count = 2000
    xz = rng.uniform(-500.0, 500.0, (count, 2)).astype(np.float32)
    oy = (surf.hmax + rng.uniform(0.0, 30.0, count)).astype(np.float32)
    rays = np.zeros((count, 6), np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 4] = xz[:, 0], oy, xz[:, 1], -1.0
    hit, nrm = R.raycast_surface(surf, rays, 200.0)
    pos, qn = surf.query(xz)
    assert np.all(hit[:, 3] >= 0.0)
    assert np.abs(hit[:, 3] - (oy - pos[:, 1])).max() <= 1e-4
    assert np.array_equal(hit[:, :3], pos[:, :3]) and np.array_equal(nrm[:, :3], qn[:, :3])
    assert np.abs(nrm[:, 3]).max() <= 1e-4


@pytest.mark.parametrize("cascades", [1, 3])
def test_oblique_rays_end_on_the_water(cascades):
    surf = surface(cascades)
    rays = oblique_rays(3000, surf, seed=2 + cascades)
    hit, nrm = R.raycast_surface(surf, rays, 2000.0)
    ok = hit[:, 3] >= 0.0
    assert ok.all()
    assert np.abs(nrm[:, 3]).max() <= 1e-4
    # the hit is on the ray: p(t).xz is where the query was made
    o, d, _ = R.unit_rays(rays)
    t = hit[:, 3]
    pos, _ = surf.query(np.stack([o[:, 0] + t * d[:, 0], o[:, 2] + t * d[:, 2]], axis=1))
    assert np.array_equal(pos[:, :3], hit[:, :3])


@pytest.mark.parametrize("cascades", [1, 3])
def test_first_crossing_agrees_with_a_brute_force_march(cascades):
    """steps = 1024 against a march 16 times denser over the same clipped segment: the first crossing lies within one brute step,
    except where the brute force found a wet interval shorter than one coarse step (the coarse march may step over it)."""
    surf = surface(cascades)
    rays = oblique_rays(120 if cascades == 1 else 60, surf, seed=11, height=(0.1, 5.0))
    rays[:, 4] *= F(0.15)                                           # grazing rays: long paths through the slab
    m, dense = 1024, 16 * 1024
    hit, _ = R.raycast_surface(surf, rays, 3000.0, steps=m)
    o, d, _ = R.unit_rays(rays)
    t0, t1, empty = R.clip(surf, o, d, 3000.0)
    assert not empty.any()
    k = np.arange(dense + 1, dtype=np.float64)[None, :]
    ts = (t0[:, None] + k * ((t1 - t0) / dense)[:, None]).astype(np.float32)
    fs = R.gap(surf, o, d, ts)
    wet = fs <= 0.0
    assert wet.any(axis=1).all()
    first = np.argmax(wet, axis=1)
    step = (t1 - t0) / dense
    tb = ts[np.arange(len(rays)), first]
    agree = np.abs(hit[:, 3] - tb) <= step * 1.01 + 1e-4
    # a thin wet interval: wet at the brute force's first crossing, dry again before the next coarse sample
    thin = np.zeros(len(rays), bool)
    for r in np.nonzero(~agree)[0]:
        nxt = min((first[r] // 16 + 1) * 16, dense)
        thin[r] = not wet[r, first[r]:nxt + 1].all() and hit[r, 3] > tb[r]
    assert (agree | thin).all(), np.nonzero(~(agree | thin))[0]
    assert agree.mean() > 0.9


def test_rays_that_miss():
    surf = surface(1)
    hm = float(surf.hmax)
    rays = np.array([
        [0.0, hm + 5.0, 0.0, 0.3, 1.0, 0.2],                    # pointing up from above the slab
        [10.0, hm + 1e-3, -4.0, 0.0, 0.5, 0.0],                 # pointing up from just above the slab
        [0.0, hm + 1.0, 0.0, 1.0, 0.0, 0.0],                    # horizontal above Hmax
        [5.0, hm, 5.0, 0.0, 0.0, -2.0],                         # horizontal at Hmax
        [0.0, hm + 50.0, 0.0, 0.0, -1.0, 0.0],                  # max_distance (40 m) ends short of the slab
        [0.0, hm + 50.0, 0.0, 0.0, 0.0, 0.0],                   # no direction
        [0.0, hm + 50.0, 0.0, np.inf, -1.0, 0.0],               # no finite direction
        [0.0, hm + 50.0, 0.0, np.nan, -1.0, 0.0],
    ], np.float32)
    hit, nrm = R.raycast_surface(surf, rays, 40.0)
    assert np.array_equal(hit, np.tile(np.array([0, 0, 0, -1], np.float32), (len(rays), 1)))
    assert np.array_equal(nrm, np.zeros_like(nrm))
    # the same vertical ray reaches the water once max_distance covers the slab
    hit, _ = R.raycast_surface(surf, rays[4:5], 60.0 + 2.0 * hm)
    assert hit[0, 3] > 50.0


def test_origins_under_water_give_the_depth():
    surf = surface(3)
    rng = np.random.default_rng(5)
    count = 500
    xz = rng.uniform(-300.0, 300.0, (count, 2)).astype(np.float32)
    pos, qn = surf.query(xz)
    depth = rng.uniform(0.01, 3.0, count).astype(np.float32)
    oy = (pos[:, 1] - depth).astype(np.float32)
    oy[:50] = -surf.hmax - F(1.0)                                   # below the slab: decided without a sample
    d = rng.normal(size=(count, 3)).astype(np.float32)             # any direction, up included
    rays = np.concatenate([xz[:, :1], oy[:, None], xz[:, 1:], d], axis=1).astype(np.float32)
    hit, nrm = R.raycast_surface(surf, rays, 100.0)
    assert np.all(hit[:, 3] == -2.0)
    assert np.array_equal(hit[:, :3], pos[:, :3]) and np.array_equal(nrm[:, :3], qn[:, :3])
    assert np.array_equal(nrm[:, 3], oy - pos[:, 1]) and np.all(nrm[:, 3] <= 0.0)


def test_settings_default_and_refine():
    """steps 0 / refine 0 are 64 / 3; more refinement rounds narrow the bracket but keep the same crossing."""
    surf = surface(1)
    rays = oblique_rays(500, surf, seed=9)
    h0, n0 = R.raycast_surface(surf, rays, 2000.0)
    h1, n1 = R.raycast_surface(surf, rays, 2000.0, steps=64, refine=3)
    assert np.array_equal(h0, h1) and np.array_equal(n0, n1)
    h8, n8 = R.raycast_surface(surf, rays, 2000.0, refine=8)
    assert np.abs(n8[:, 3]).max() <= np.abs(n0[:, 3]).max() + 1e-6
    assert np.abs(h8[:, 3] - h0[:, 3]).max() <= 1e-2


def flat_surface(n=32):
    """What a context with phillips_const = 0 renders (tests/test_parity_gpu.py::test_zero_spectrum_minmax_quirk): height 0, w = 1, every
    other channel 0, and the amplitude FLT_MIN."""
    disp = np.zeros((n, n, 4), np.float32)
    disp[..., 3] = 1.0
    return R.Surface([disp], [np.zeros((n, n, 4), np.float32)], [float(np.finfo(np.float32).tiny)], [-1.0], [1000.0], [1.0],
                     512, 1000.0 / 512, -1.0)


@pytest.mark.parametrize("steps,refine", [(0, 0), (1, 1), (17, 8)])
def test_a_flat_sea_is_hit_by_every_downward_ray(steps, refine):
    """Calm water is a picking target.  With Hmax = 1.001 * FLT_MIN the slab had no thickness, every sample was the one point
    o.y + t0 * d.y, and its rounding turned about 4 % of these rays into misses at every setting; the slab's 1 mm floor lets the march
    bracket the plane.  400 m of reach cover the shallowest ray (30 m up, 5 degrees down: 344 m).  The kernel's twin of this test is
    tests/test_surface_raycast_edges_gpu.py::test_a_flat_sea_is_hit_by_every_downward_ray."""
    surf = flat_surface()
    assert surf.hmax == F(1e-3)
    rays = R.flat_sea_rays()
    assert len(rays) % 16 != 0
    hit, nrm = R.raycast_surface(surf, rays, 400.0, steps, refine)
    gap_ulps, t_err = R.check_flat_sea(rays, hit, nrm, (steps, refine))
    print(f"flat sea steps={steps} refine={refine}: {len(rays)} hits, gap <= {gap_ulps:.2f} ulp(o.y), t off by <= {t_err:.3g}")


def test_rays_at_the_surface_of_a_flat_sea():
    near = np.array([r for r, _ in R.NEAR_SURFACE], np.float32)
    R.check_near_surface(*R.raycast_surface(flat_surface(), near, 40.0))


@pytest.fixture(scope="module")
def abi():
    from watersurfacerendering_amd import _abi
    _abi.build()
    return _abi


def test_raycast_abi_checks_arguments_without_a_device(abi):
    L = abi.lib()
    s = abi.Surface()
    s.cascades, s.grid_size = 1, 64
    r = abi.Raycast()
    r.max_distance = 100.0
    assert C.sizeof(abi.Raycast) == 12
    assert L.ocean_raycast_surface(None, C.byref(s), C.byref(r), None, 0, None, None) == abi.OCEAN_E_INVALID
    assert L.ocean_raycast_surface_device(None, C.byref(s), C.byref(r), None, 0, None, None) == abi.OCEAN_E_INVALID
    assert L.ocean_raycast_surface(None, None, C.byref(r), None, 0, None, None) == abi.OCEAN_E_INVALID
    assert L.ocean_raycast_surface(None, C.byref(s), None, None, 0, None, None) == abi.OCEAN_E_INVALID


def test_cpp_adaptor_raycast_surface_builds(abi, tmp_path):
    """tests/cpp/raycast_demo.cpp (WSTessendorf::RaycastSurface) compiles and links against the C ABI; without a GPU it fails loudly."""
    exe = tmp_path / "raycast_demo"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "raycast_demo.cpp"), "-o", str(exe),
                    "-L", os.path.dirname(abi.LIB_PATH), "-locean_hip", "-Wl,-rpath," + os.path.dirname(abi.LIB_PATH),
                    "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([str(exe), "64", str(tmp_path / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 3 and "no usable HIP device" in r.stderr
