"""Surface query on the MI355X (include/ocean_consumers.h: ocean_query_surface / ocean_query_surface_device): the HIP kernel
against the float32 restatement (tests/surface_query.py) on maps read back from the same frame, against the vertex stage on the
GPU, and the API's ordering, bound output, size and error rules."""
import os
import subprocess

import numpy as np
import pytest

import surface_query as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LENGTHS3 = [1000.0, 370.0, 93.0]        # the cascade set of tests/test_consumer.py::test_cascade_consumer_matches_oracle_on_tiles_of_different_length


def _points(kind, count, half, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.uniform(-half, half, (count, 2)).astype(np.float32)
    side = int(np.sqrt(count))                                     # coherent: a jittered grid, row by row
    g = (np.arange(side, dtype=np.float32) + 0.5) * np.float32(2 * half / side) - np.float32(half)
    xz = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)
    return (xz + rng.uniform(-0.4, 0.4, xz.shape) * np.float32(2 * half / side)).astype(np.float32)


def _compare(pos, nrm, opos, onrm, total_tag):
    """Every point where both residuals are < 1e-3 m agrees to 1e-5 of the channel's magnitude (the residual: of the xz position
    range, both in metres); a point may go to another root only where the restatement's residual is >= 1e-3 m, and those are
    < 0.1 % of the points.  Returns the number of bit-identical points."""
    got, want = np.concatenate([pos, nrm], 1), np.concatenate([opos, onrm], 1)
    scale = np.abs(want).max(0)
    scale[7] = scale[[0, 2]].max()
    scale = np.maximum(scale, 1e-30)
    close = np.all(np.abs(got - want) <= 1e-5 * scale, axis=1)
    both = (nrm[:, 3] < 1e-3) & (onrm[:, 3] < 1e-3)
    assert close[both].all(), (total_tag, int((~close & both).sum()))
    other = ~close
    assert not (other & (onrm[:, 3] < 1e-3)).any(), (total_tag, int((other & (onrm[:, 3] < 1e-3)).sum()))
    assert other.sum() < 1e-3 * len(pos), (total_tag, int(other.sum()))
    return int(np.all(got.view(np.uint32) == want.view(np.uint32), axis=1).sum())


@pytest.mark.parametrize("n,cascades", [(64, 1), (64, 3), (512, 1), (512, 3), (2048, 1), (2048, 3)])
def test_kernel_matches_restatement(n, cascades):
    import watersurfacerendering_amd as W
    lengths = [1000.0] if cascades == 1 else LENGTHS3
    b = W.OceanBatch(n, len(lengths), 0)
    for i, L in enumerate(lengths):
        b.set_params(tile=i, tile_length=L)
    b.prepare(0x5EED0000 + n)
    amps = [float(a) for a in b.compute_waves(3.7)]
    disp, nrm = b.read_maps()
    grid = 512
    vd = lengths[0] / grid
    scales = [lengths[0] / L for L in lengths]                     # every cascade keeps its metres per texel
    for kind in ("random", "grid"):
        xz = _points(kind, 4096 if n == 2048 else 16384, 700.0, seed=n)
        for k in (1, 8, 32):
            pos, nr = b.query_surface(xz, 0, scales, grid, vd, -1.0, k)
            opos, onr = S.query_surface(list(disp), list(nrm), amps, [-1.0] * len(lengths), lengths, scales, grid, vd, -1.0, xz, k)
            same = _compare(pos, nr, opos, onr, (n, cascades, kind, k))
            print(f"n={n} cascades={cascades} {kind} K={k}: {same}/{len(xz)} points bit-identical; "
                  f"residual p99 {np.quantile(nr[:, 3], 0.99):.3g} m")
    b.close()


@pytest.mark.parametrize("cascades", [1, 3])
def test_round_trip_against_the_vertex_stage(cascades):
    """OCEAN_MODE_JACOBIAN: the vertex stage runs on the GPU, then the query at the displaced xz of every vertex whose Jacobian slot is
    > 0.3 gives back that vertex's position and normal."""
    import watersurfacerendering_amd as W
    n, grid = 256, 256
    lengths = [1000.0] if cascades == 1 else LENGTHS3
    b = W.OceanBatch(n, len(lengths), 0)
    for i, L in enumerate(lengths):
        b.set_params(tile=i, tile_length=L)
    b.set_mode(W._abi.OCEAN_MODE_JACOBIAN)
    b.prepare(11)
    amps = b.compute_waves(3.7)
    vd = lengths[0] / grid
    scales = [lengths[0] / L for L in lengths]
    if cascades == 1:
        pv, nv = b.displace_grid(0, grid, vd, 1.0, -1.0)
    else:
        pv, nv = b.displace_grid_cascades(scales, 0, grid, vd, -1.0)
    sel = pv[:, 3] > 0.3
    assert sel.mean() > 0.9
    pos, nr = b.query_surface(pv[sel][:, [0, 2]], 0, scales, grid, vd, -1.0, 32)
    a = float(np.max(amps))
    assert np.abs(pos[:, [0, 2]] - pv[sel][:, [0, 2]]).max() <= 1e-3
    assert np.abs(pos[:, 1] - pv[sel][:, 1]).max() <= 1e-4 * a
    assert np.abs(nr[:, :3] - nv[sel][:, :3]).max() <= 1e-4
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
    xz = _points("random", 100000, 800.0, 1)
    pos, nr = b.query_surface(xz, iterations=8)
    d_xz = torch.from_numpy(xz).cuda()
    d_pos = torch.empty((len(xz), 4), dtype=torch.float32, device="cuda")
    d_nrm = torch.empty_like(d_pos)
    torch.cuda.synchronize()
    b.query_surface_device(d_xz.data_ptr(), len(xz), d_pos.data_ptr(), d_nrm.data_ptr(), iterations=8)
    b.synchronize()
    assert np.array_equal(d_pos.cpu().numpy(), pos) and np.array_equal(d_nrm.cpu().numpy(), nr)
    b.close()


def test_pipelined_context_answers_for_its_most_recent_frame():
    import watersurfacerendering_amd as W
    xz = _points("random", 20000, 800.0, 2)
    s = _batch(512, seed=9, t=2.5)
    want = s.query_surface(xz)
    s.close()
    p = W.OceanBatch(512, 1, 0)
    p.set_pipeline_depth(3)
    p.prepare(9)
    for t in (0.5, 1.5, 2.5):
        p.compute_waves_async(t)
    got = p.query_surface(xz)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    p.close()


def test_query_reads_caller_bound_maps():
    import torch
    import watersurfacerendering_amd as W
    n = 128
    xz = _points("random", 5000, 500.0, 3)
    ref = _batch(n, seed=21)
    want = ref.query_surface(xz)
    ref.close()
    maps = torch.zeros((2, n, n, 4), dtype=torch.float32, device="cuda")
    b = W.OceanBatch(n, 1, 0)
    b.bind_output(maps[0].data_ptr(), maps[1].data_ptr())
    b.prepare(21)
    b.compute_waves(3.7)
    got = b.query_surface(xz)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    b.synchronize()
    maps.zero_()                        # the query reads the bound memory where it is: flat water from now on
    torch.cuda.synchronize()
    pos, nr = b.query_surface(xz)
    assert np.array_equal(pos[:, [0, 2]], xz) and np.all(pos[:, 1] == 0.0) and np.all(pos[:, 3] == 0.0)
    assert np.all(nr[:, :3] == np.array([0.0, 1.0, 0.0], np.float32)) and np.all(nr[:, 3] == 0.0)
    b.bind_output(None, None)
    b.close()


def test_four_million_points_in_one_call():
    b = _batch(512, seed=4)
    count = 1 << 22
    xz = _points("random", count, 2000.0, 4)
    pos, nr = b.query_surface(xz)
    assert pos.shape == (count, 4) and np.isfinite(pos).all() and np.isfinite(nr).all()
    idx = np.random.default_rng(0).choice(count, 4096, replace=False)
    idx.sort()
    p2, n2 = b.query_surface(xz[idx])
    assert np.array_equal(p2, pos[idx]) and np.array_equal(n2, nr[idx])
    assert np.median(nr[:, 3]) < 1e-4
    b.close()


def test_argument_and_readiness_errors():
    import ctypes as C
    import watersurfacerendering_amd as W
    A = W._abi
    b = W.OceanBatch(64, 2, 0)
    xz = _points("random", 16, 100.0)
    with pytest.raises(W.OceanError) as e:
        b.query_surface(xz)                                 # nothing prepared
    assert e.value.code == A.OCEAN_E_NOT_READY
    b.prepare(3)
    with pytest.raises(W.OceanError) as e:
        b.query_surface(xz)                                 # no frame yet
    assert e.value.code == A.OCEAN_E_NOT_READY
    b.compute_waves(1.0)
    for kw in (dict(uv_scales=(1.0,) * 3), dict(first_tile=2), dict(first_tile=1, uv_scales=(1.0, 1.0)), dict(grid_size=0),
               dict(iterations=33)):
        with pytest.raises(W.OceanError) as e:
            b.query_surface(xz, **kw)
        assert e.value.code == A.OCEAN_E_INVALID, kw
    L, s = b._L, b._surface(0, (1.0,), None, None, -1.0, 8)
    s.cascades = 0
    assert L.ocean_query_surface(b._h, C.byref(s), None, 0, None, None) == A.OCEAN_E_INVALID
    s.cascades = 9
    assert L.ocean_query_surface(b._h, C.byref(s), None, 0, None, None) == A.OCEAN_E_INVALID
    s.cascades = 1
    assert L.ocean_query_surface(b._h, None, None, 0, None, None) == A.OCEAN_E_INVALID
    assert L.ocean_query_surface(b._h, C.byref(s), None, 4, None, None) == A.OCEAN_E_INVALID
    assert L.ocean_query_surface_device(b._h, C.byref(s), None, 4, None, None) == A.OCEAN_E_INVALID
    assert L.ocean_query_surface(b._h, C.byref(s), None, 0, None, None) == A.OCEAN_OK           # points = 0: nothing to do
    assert L.ocean_query_surface_device(b._h, C.byref(s), None, 0, None, None) == A.OCEAN_OK
    pos, _ = b.query_surface(xz, first_tile=1, uv_scales=(1.0,), iterations=32)
    assert pos.shape == (16, 4)
    b.close()


def test_a_later_lambda_does_not_change_the_answer():
    """The Newton step uses the lambda of the frame that wrote the maps; ocean_set_lambda only changes the NEXT frame."""
    b = _batch(256, seed=8)
    xz = _points("random", 20000, 600.0, 5)
    want = b.query_surface(xz)
    b.set_lambda(-2.0)
    got = b.query_surface(xz)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    b.compute_waves(3.7)                                    # a frame with the new lambda: a different surface
    assert not np.array_equal(b.query_surface(xz)[0], want[0])
    b.close()


def test_cpp_adaptor_query_matches_python_binding(tmp_path):
    import watersurfacerendering_amd as W
    from watersurfacerendering_amd import _abi
    exe = tmp_path / "query_demo"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "query_demo.cpp"), "-o", str(exe),
                    "-L", os.path.dirname(_abi.LIB_PATH), "-locean_hip", "-Wl,-rpath," + os.path.dirname(_abi.LIB_PATH),
                    "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = tmp_path / "query.bin"
    r = subprocess.run([str(exe), "128", str(out), "3.7"], capture_output=True, text=True, check=True)
    n, amp, points, worst = r.stdout.split()
    points = int(points)
    raw = np.fromfile(out, dtype=np.float32)
    xz = raw[:2 * points].reshape(points, 2)
    cpos = raw[2 * points:6 * points].reshape(points, 4)
    cnrm = raw[6 * points:].reshape(points, 4)
    ws = W.WSTessendorf(128, 1000.0)
    ws.SetWindDirection((1.0, 0.5)); ws.SetWindSpeed(20.0); ws.SetLambda(-1.5)
    ws.Prepare(seed=42)
    assert ws.ComputeWaves(3.7) == pytest.approx(float(amp), rel=1e-7)
    pos, nrm = ws.QuerySurface(xz)
    assert np.array_equal(pos, cpos) and np.array_equal(nrm, cnrm)
    assert float(worst) == float(nrm[:, 3].max())
