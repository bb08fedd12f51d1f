"""The fragment stage on the MI355X (ocean_sky_radiance, ocean_eval_seabed, ocean_shade_points, ocean_shade_grid and their device forms)
against tests/shading.py: the seabed noise in every bit, the optics within twice the derived bound B per channel, out_aux within its own
bound, the reference seabed through the device's own seabed hit, forms and bits, the grid "as rendered", readiness and errors.  The largest
error / B ratios seen on the device are in the docstring of test_shade_points_within_the_bound."""
import ctypes as C

import numpy as np
import pytest

import shading as S

pytestmark = pytest.mark.gpu
f32 = np.float32
E_INVALID, E_NOT_READY = -1, -4
SKY = dict(sun_color=(1.0, 1.0, 1.0), sun_intensity=f32(1.0))
SEABED_COUNTS = (1, 63, 64, 65, 255, 256, 257, 4099)
F0 = f32(((S.IOR - 1.0) / (S.IOR + 1.0)) ** 2)


def W():
    import watersurfacerendering_amd as w
    return w


@pytest.fixture(scope="module")
def batch():
    b = W().OceanBatch(64, 3)
    yield b
    b.close()


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def empty(rows):
    import torch
    t = torch.full((rows, 4), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return t


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def ratio_of(got, want, bound):
    """error / B per element; 0 where both the error and the bound are 0 (foam rows, exact constants)."""
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(all="ignore"):
        return np.where(err == 0.0, 0.0, err / bound)


# ---- seabed: every bit ------------------------------------------------------------------------------------------------------------------------
def seabed_points(count, seed=2):
    rng = np.random.default_rng(seed)
    crafted = np.array([[0, 0], [-0.0, 0.0], [50, 100], [-150, 50], [25, -25], [1e4, -1e4], [-1e4, 1e4], [9999.5, 0.25], [-3.75, -8.125], [1e-3, -1e-3],
                        [2048, 2048], [0.5, 1e4]], dtype=np.float64)          # 50 m is one cell of the first octave: exact integers of the scaled lattice
    rnd = np.concatenate([rng.uniform(-1e4, 1e4, (count, 2)), rng.uniform(-80, 80, (count, 2)), 50.0 * rng.integers(-200, 200, (count, 2))])
    return np.concatenate([crafted, rnd[rng.permutation(len(rnd))]])[:count].astype(f32)


@pytest.mark.parametrize("count", SEABED_COUNTS)
def test_seabed_bit_for_bit(batch, count):
    xz = seabed_points(count)
    want = S.seabed(xz)
    got = batch.eval_seabed(xz)
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    assert bad.size == 0, (count, int(bad[0]), xz[bad[0]], got[bad[0]], want[bad[0]])
    out, d_xz = empty(count), dev(xz)
    batch.eval_seabed_device(d_xz, count, out)
    batch.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


# ---- sky radiance ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("turbidity", S.TURBIDITIES)
@pytest.mark.parametrize("si", range(3))
def test_sky_radiance_within_the_bound(batch, si, turbidity):
    """4099 directions (zenith, horizon, below it, the sun, rings across both smoothstep edges) within 2 B per channel.  Largest error / B
    seen on the device: see test_shade_points_within_the_bound."""
    w = W()
    sun, color = S.SUNS[si], (1.0, 0.9, 0.8)
    sky = w.sky_params(sun_dir=sun, turbidity=turbidity, sun_color=color)
    co = S.coefficients_of(w.sky_coefficients(sky))
    dirs = S.sky_directions(sun)
    want, bound = S.sky_radiance(co, color, dirs)
    got = batch.sky_radiance(dirs, sky)
    assert np.isfinite(want).all() and np.isfinite(got).all()
    r = ratio_of(got, want, bound)
    print(f"sky sun{si} T={turbidity}: largest error / B {r.max(axis=0)}")
    assert (r <= 2.0).all(), (si, turbidity, float(r.max()), int(np.argmax(r.max(axis=1))))
    out, d_dirs = empty(len(dirs)), dev(dirs)
    batch.sky_radiance_device(d_dirs, len(dirs), out, sky)
    batch.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(got))


# ---- water colour ----------------------------------------------------------------------------------------------------------------------------
def held(batch, sun, pos, nrm, what, seabed_rows=False, **fields):
    """Shades (pos, nrm) on the device and restates it; returns (rgba ratio, aux ratio, got rgba, got aux, restated)."""
    w = W()
    sky = w.sky_params(sun_dir=sun)
    co = S.coefficients_of(w.sky_coefficients(sky))
    water = w.water_params(cam_pos=S.CAM, **fields)
    rgba, aux = batch.shade_points(pos, nrm, sky, water, aux=True)
    rows = S.seabed(aux[:, :2]) if seabed_rows else None          # the noise at the device's own seabed hit
    want = S.shade(co, SKY, S.water_dict(water), pos, nrm, seabed_rows=rows)
    ok = np.isfinite(want["rgba"]).all(axis=1) & np.isfinite(want["aux"]).all(axis=1) & ~want["ambiguous"]
    assert ok.mean() > 0.99, (what, float(ok.mean()))
    r = ratio_of(rgba, want["rgba"], want["rgba_bound"])[ok]
    ra = ratio_of(aux, want["aux"], want["aux_bound"])[ok]
    print(f"{what}: largest error / B: rgba {r.max(axis=0)}, aux {ra.max(axis=0)}")
    assert (r <= 2.0).all(), (what, float(r.max()), int(np.argmax(r.max(axis=1))))
    assert (ra <= 2.0).all(), (what, float(ra.max()), int(np.argmax(ra.max(axis=1))))
    return r, ra, rgba, aux, want


@pytest.mark.parametrize("fresnel", (0, 1))
@pytest.mark.parametrize("wi", (0, 1))
@pytest.mark.parametrize("si", range(3))
def test_shade_points_within_the_bound(batch, si, wi, fresnel):
    """FLAT seabed, not tone-mapped, both Fresnel kinds, three suns, two waters, 4000 random vertices and the crafted rows (normal incidence,
    grazing views, back-facing normals, mirrors into the sun and rings across the disk's edges, foam): colour and out_aux within 2 B.
    Largest error / B seen on the MI355X, per family -- water colour 0.17 (FLAT seabed, either Fresnel), highlights 512: 0.14,
    tone-mapped 0.17, frame rows 0.14, reference seabed 0.18, sky radiance 0.24; out_aux 0.99 in p_g (where B is almost only the
    rounding of the output itself: half an ulp against 2^-24 |v|), 0.25 in t_g, 0.18 in F_r.  No family exceeds 1: the assumed four
    ulps per transcendental are not exceeded anywhere the inputs reach."""
    sun = S.SHADE_SUNS[si]
    pos, nrm, tags = S.shade_rows(sun)
    r, ra, rgba, aux, want = held(batch, sun, pos, nrm, f"sun{si} water{wi} fresnel{fresnel}", seabed=1, tonemap=0, fresnel=fresnel,
                                  **S.water_fields(S.WATERS[wi]))
    assert (rgba[:, 3] == 1.0).all()
    foam = pos[:, 3] < 0
    assert (rgba[foam, :3] == 1.0).all() and (rgba[~foam, :3] != 1.0).any()
    back = slice(*tags["backfacing"])
    if fresnel == 0:
        assert (aux[back, 3] == F0).all(), aux[back, 3]               # dot(n, V) <= 1e-5: the shader's first branch, rounded once
    else:
        assert (aux[back, 3] == 1.0).all()
        above = slice(*tags["above"])
        assert np.abs(aux[above, 3].astype(np.float64) - float(F0)).max() < 1e-7            # normal incidence: the same reflectance, computed


def test_shade_points_highlights_tonemap_and_foam_switch(batch):
    sun = S.SHADE_SUNS[0]
    pos, nrm, tags = S.shade_rows(sun)
    held(batch, sun, pos, nrm, "highlights 512", seabed=1, tonemap=0, specular_highlights=512.0)
    _, _, tm, _, _ = held(batch, sun, pos, nrm, "tone-mapped", seabed=1, tonemap=1)
    assert np.abs(tm[:, 3] - (1.0 - np.exp(-2.0))).max() < 3e-7
    _, _, off, _, _ = held(batch, sun, pos, nrm, "foam_white 0", seabed=1, tonemap=0, foam_white=0)
    foam = pos[:, 3] < 0
    assert (off[foam, :3] != 1.0).all()


def test_shade_points_on_a_real_frame(batch):
    """The vertex stage's output of a 64 x 64 frame on a grid of 64 x 64 vertices, as ocean_displace_grid writes it."""
    batch.set_params(phillips_const=5e-8)
    batch.prepare(seed=0x5EA)
    batch.compute_waves(3.0)
    pos, nrm = batch.displace_grid(0, 63, 4.0)
    assert pos.shape == (4096, 4) and np.abs(pos[:, 1]).max() > 0.05
    held(batch, S.SHADE_SUNS[0], pos, nrm, "frame rows", seabed=1, tonemap=0)
    held(batch, S.SHADE_SUNS[1], pos, nrm, "frame rows, physical", seabed=1, tonemap=0, fresnel=1)


@pytest.mark.parametrize("si", range(3))
def test_reference_seabed_through_the_devices_own_hit(batch, si):
    """OCEAN_SEABED_REFERENCE: (p_g.x, p_g.z) from the device's out_aux, the float32 noise there (bit-equal to ocean_eval_seabed, checked
    here again), injected into the float64 restatement: the colour within 2 B."""
    sun = S.SHADE_SUNS[si]
    pos, nrm, _ = S.shade_rows(sun)
    _, _, _, aux, _ = held(batch, sun, pos, nrm, f"reference seabed sun{si}", seabed_rows=True, seabed=0, tonemap=0)
    assert np.array_equal(bits(batch.eval_seabed(aux[:, :2])), bits(S.seabed(aux[:, :2])))
    flat = batch.shade_points(pos, nrm, W().sky_params(sun_dir=sun), W().water_params(cam_pos=S.CAM, seabed=1, tonemap=0))
    ref = batch.shade_points(pos, nrm, W().sky_params(sun_dir=sun), W().water_params(cam_pos=S.CAM, seabed=0, tonemap=0))
    assert (flat != ref).any()


def test_forms_bits_and_rows_that_do_not_disturb(batch):
    w = W()
    sun = S.SHADE_SUNS[1]
    sky, water = w.sky_params(sun_dir=sun), w.water_params(cam_pos=S.CAM)
    pos, nrm, _ = S.shade_rows(sun)
    rgba, aux = batch.shade_points(pos, nrm, sky, water, aux=True)
    again, aux2 = batch.shade_points(pos, nrm, sky, water, aux=True)
    assert np.array_equal(bits(rgba), bits(again)) and np.array_equal(bits(aux), bits(aux2))
    assert np.array_equal(bits(batch.shade_points(pos, nrm, sky, water)), bits(rgba))          # without out_aux
    d_rgba, d_aux, d_pos, d_nrm = empty(len(pos)), empty(len(pos)), dev(pos), dev(nrm)
    batch.shade_points_device(d_pos, d_nrm, len(pos), d_rgba, d_aux, sky, water)
    batch.synchronize()
    assert np.array_equal(bits(d_rgba.cpu().numpy()), bits(rgba)) and np.array_equal(bits(d_aux.cpu().numpy()), bits(aux))
    d_only = empty(len(pos))
    batch.shade_points_device(d_pos, d_nrm, len(pos), d_only, None, sky, water)
    batch.synchronize()
    assert np.array_equal(bits(d_only.cpu().numpy()), bits(rgba))
    # a zero normal, a NaN position, pos == cam, an infinite normal: their rows are unspecified, every other row is as it was
    bad_pos, bad_nrm = pos.copy(), nrm.copy()
    rows = [5, 64, 255, 1000]
    bad_nrm[5, :3] = 0.0
    bad_pos[64, 0] = np.nan
    bad_pos[255, :3] = S.CAM
    bad_nrm[1000, 1] = np.inf
    got, gaux = batch.shade_points(bad_pos, bad_nrm, sky, water, aux=True)
    keep = np.ones(len(pos), dtype=bool)
    keep[rows] = False
    assert np.array_equal(bits(got[keep]), bits(rgba[keep])) and np.array_equal(bits(gaux[keep]), bits(aux[keep]))


def test_shade_grid_is_shade_points_on_the_grid(batch):
    """Grid sizes 1, 15, 16, 64 behind ocean_displace_grid, _cascades with 3 tiles and _lod: the image equals ocean_shade_points_device on
    ocean_device_grid's buffers in every bit; ocean_read_shaded round-trips; OCEAN_E_NOT_READY before any grid and after ocean_prepare."""
    w = W()
    b = w.OceanBatch(64, 3)
    sky = w.sky_params(sun_dir=S.SHADE_SUNS[0])
    scales = (1.0, 1.7, 0.45)
    code = lambda: b._L.ocean_shade_grid(b._h, C.byref(sky), C.byref(w.water_params()))
    assert code() == E_NOT_READY                      # nothing prepared
    b.set_params(phillips_const=5e-8)
    b.prepare(seed=7)
    assert code() == E_NOT_READY                      # no frame, no grid
    b.compute_waves(1.0)
    assert code() == E_NOT_READY                      # a frame, but no grid yet
    assert b.device_shaded() == (None, 0)
    with pytest.raises(w.OceanError) as e:
        b.read_shaded()
    assert e.value.code == E_NOT_READY
    for grid in (1, 15, 16, 64):
        for how in ("grid", "cascades", "lod"):
            for seabed in (0, 1):
                water = w.water_params(cam_pos=(5.0, 30.0, -20.0), seabed=seabed)
                if how == "grid":
                    pos, nrm = b.displace_grid(1, grid, 3.0)
                elif how == "cascades":
                    pos, nrm = b.displace_grid_cascades(scales, 0, grid, 3.0)
                else:
                    b.build_mips_tiles(0, 3)
                    pos, nrm = b.displace_grid_lod(scales, 0, grid, 40.0)
                b.shade_grid(sky, water)
                image = b.read_shaded()
                d_pos, d_nrm, verts = b.device_grid()
                assert verts == (grid + 1) ** 2 == len(image) and b.device_shaded()[1] == verts
                out = empty(verts)
                b.shade_points_device(d_pos, d_nrm, verts, out, None, sky, water)
                b.synchronize()
                assert np.array_equal(bits(out.cpu().numpy()), bits(image)), (grid, how, seabed)
                assert np.array_equal(bits(b.shade_points(pos, nrm, sky, water)), bits(image)), (grid, how, seabed)
                assert np.isfinite(image).all() and (image[:, 3] == image[0, 3]).all()
    b.prepare(seed=8)
    assert code() == E_NOT_READY                      # the grid belonged to the old sea
    b.compute_waves(0.5)
    b.displace_grid(0, 16, 3.0)
    b.shade_grid(sky)
    assert len(b.read_shaded()) == 17 * 17
    b.close()


def test_errors(batch):
    w = W()
    L, h = batch._L, batch._h
    sky, water = w.sky_params(), w.water_params()
    one = np.zeros((1, 4), dtype=f32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    shade = lambda s, wt, pos=one, nrm=one, out=one, n=1: L.ocean_shade_points(h, None if s is None else C.byref(s), None if wt is None else C.byref(wt),
                                                                                None if pos is None else p(pos), None if nrm is None else p(nrm), n,
                                                                                None if out is None else p(out), None)
    assert shade(sky, water) == 0
    assert [shade(None, water), shade(sky, None), shade(sky, water, pos=None), shade(sky, water, nrm=None), shade(sky, water, out=None)] == [E_INVALID] * 5
    assert L.ocean_shade_points(None, C.byref(sky), C.byref(water), p(one), p(one), 1, p(one), None) == E_INVALID
    assert shade(sky, water, pos=None, nrm=None, out=None, n=0) == 0                    # count == 0: before the pointers are looked at
    nan, inf = float("nan"), float("inf")
    bad_water = [dict(absorb=(0.0, 0.1, 0.1)), dict(absorb=(0.1, -0.1, 0.1)), dict(specular_highlights=0.0), dict(specular_highlights=-1.0),
                 dict(fresnel=2), dict(seabed=2), dict(height=nan), dict(cam_pos=(0, inf, 0)), dict(scatter=(nan, 0, 0)), dict(backscatter=(0, 0, inf)),
                 dict(terrain_color=(nan, 1, 1)), dict(sky_intensity=inf), dict(specular_intensity=nan), dict(seabed_factor=nan), dict(absorb=(nan, 1, 1))]
    for fields in bad_water:
        assert shade(sky, w.water_params(**fields)) == E_INVALID, fields
        assert L.ocean_shade_grid(h, C.byref(sky), C.byref(w.water_params(**fields))) == E_INVALID, fields
    bad_sky = [dict(turbidity=0.5), dict(turbidity=10.01), dict(turbidity=nan), dict(sun_dir=(0, 0, 0)), dict(sun_dir=(nan, 1, 0)), dict(sun_color=(1, inf, 1)),
               dict(sun_intensity=nan)]
    dirs, out = np.array([[0, 1, 0]], dtype=f32), np.zeros((1, 4), dtype=f32)
    for fields in bad_sky:
        s = w.sky_params(**fields)
        assert shade(s, water) == E_INVALID, fields
        assert L.ocean_sky_radiance(h, C.byref(s), p(dirs), 1, p(out)) == E_INVALID, fields
        assert L.ocean_sky_radiance_device(h, C.byref(s), p(dirs), 0, None) == E_INVALID, fields
    assert L.ocean_sky_radiance(h, C.byref(sky), None, 1, p(out)) == E_INVALID and L.ocean_sky_radiance(h, C.byref(sky), p(dirs), 1, None) == E_INVALID
    assert L.ocean_sky_radiance(h, None, p(dirs), 1, p(out)) == E_INVALID and L.ocean_sky_radiance(None, C.byref(sky), p(dirs), 1, p(out)) == E_INVALID
    assert L.ocean_sky_radiance(h, C.byref(sky), None, 0, None) == 0 and L.ocean_sky_radiance_device(h, C.byref(sky), None, 0, None) == 0
    xz = np.zeros((1, 2), dtype=f32)
    assert L.ocean_eval_seabed(h, None, 1, p(out)) == E_INVALID and L.ocean_eval_seabed(h, p(xz), 1, None) == E_INVALID
    assert L.ocean_eval_seabed(None, p(xz), 1, p(out)) == E_INVALID
    assert L.ocean_eval_seabed(h, None, 0, None) == 0 and L.ocean_eval_seabed_device(h, None, 0, None) == 0
    assert L.ocean_shade_points_device(h, C.byref(sky), C.byref(water), None, None, 1, None, None) == E_INVALID
    assert L.ocean_shade_points_device(h, C.byref(sky), C.byref(water), None, None, 0, None, None) == 0
    assert L.ocean_shade_grid(None, C.byref(sky), C.byref(water)) == E_INVALID and L.ocean_shade_grid(h, None, C.byref(water)) == E_INVALID
    assert L.ocean_read_shaded(None, p(out)) == E_INVALID and L.ocean_read_shaded(h, None) == E_INVALID
    assert L.ocean_device_shaded(None, None, None) == E_INVALID


def test_sky_and_seabed_need_no_prepare():
    """ocean_sky_radiance and ocean_eval_seabed use the context for its stream and staging only."""
    b = W().OceanBatch(16, 1)
    got = b.sky_radiance(np.array([[0.0, 1.0, 0.0], [1.0, 0.2, 0.0]], dtype=f32))
    assert np.isfinite(got).all() and (got[:, :3] > 0).all()
    assert np.array_equal(bits(b.eval_seabed(seabed_points(65))), bits(S.seabed(seabed_points(65))))
    rgba = b.shade_points(np.array([[10.0, 0.0, 5.0, 1.0]], dtype=f32), np.array([[0.0, 1.0, 0.0, 0.0]], dtype=f32))
    assert np.isfinite(rgba).all()
    b.close()


def test_cpp_host_matches_the_python_binding(tmp_path):
    """tests/cpp/shading_demo.cpp: the grid "as rendered" through the C ABI from C++, bit for bit what the binding returns."""
    import os
    import subprocess
    w = W()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.dirname(w._abi.LIB_PATH)
    exe = tmp_path / "shading_demo"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "shading_demo.cpp"),
                    "-o", str(exe), "-L", lib, "-locean_hip", "-Wl,-rpath," + lib, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = tmp_path / "shaded.bin"
    r = subprocess.run([str(exe), "64", str(out), "2.0"], capture_output=True, text=True, check=True)
    n, vertices, checksum, zenith = r.stdout.split()
    image = np.fromfile(out, dtype=f32).reshape(-1, 4)
    assert int(n) == 64 and int(vertices) == 65 * 65 == len(image)
    assert float(checksum) == pytest.approx(float(image.astype(np.float64).sum()), rel=1e-8)
    assert float(zenith) == pytest.approx(float(w.sky_coefficients().zenith_lum[0]), rel=1e-7)
    b = w.OceanBatch(64, 1)
    b.prepare(seed=42)
    b.compute_waves(2.0)
    p = b.get_params(0)
    b.displace_grid(0, 64, p.tile_length / f32(64), 1.0, p.lambda_)
    b.shade_grid()
    assert np.array_equal(bits(b.read_shaded()), bits(image))
    assert np.isfinite(image).all() and (image < 1).all() and image[:, :3].mean() > 0.05           # tone-mapped: below 1
    b.close()
