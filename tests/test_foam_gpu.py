"""Persistent foam on the MI355X (include/ocean_consumers.h: ocean_update_foam, ocean_query_foam ...): the HIP kernels against the float32
restatement (tests/foam.py) on maps read back from the same frames -- synthesis error does not enter, so equality is the expectation --,
and the API's ordering, selection, lifetime, bound-output and error rules."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import foam as FM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
LENGTHS3 = [1000.0, 370.0, 93.0]        # the cascade set of tests/test_surface_query_gpu.py
DT = 0.1


def _time(j):
    return float(np.float32(0.1) * np.float32(j))


def _run_against_restatement(b, tiles, steps, p_kw, share_bounds, from_slot, tag, lambdas=None):
    """`steps` frames t_j = 0.1 j with one update behind each; the restatement runs on the maps read back from the same frames.  The
    share of generating texels of every tile is asserted on every compared frame; foam is compared after every 5th step and at the end."""
    n = b.tile_size
    p = FM.params(**p_kw)
    dec = FM.decay(DT, p["lifetime"])
    lambdas = [-1.0] * tiles if lambdas is None else lambdas
    want = [np.zeros((n, n), np.float32) for _ in range(tiles)]
    for j in range(steps):
        b.compute_waves(_time(j))
        b.update_foam(DT, **p_kw)
        disp, nrm = b.read_maps()
        compared = (j + 1) % 5 == 0 or j + 1 == steps
        for i in range(tiles):
            jac = FM.jacobian(disp[i], nrm[i], lambdas[i], from_slot)
            want[i] = FM.step(want[i], jac, p, dec)
            if compared:
                share = float((FM.generation(jac, p) > 0).mean())
                print(f"{tag} step {j + 1} tile {i}: generating share {share:.4f}, mean foam {float(want[i].mean()):.4f}")
                assert share_bounds[0] <= share <= share_bounds[1], (tag, j + 1, i, share)
                got = b.read_foam(i)
                assert np.array_equal(got, want[i]), (tag, j + 1, i, int((got != want[i]).sum()), float(np.abs(got - want[i]).max()))
    for i in range(tiles):
        assert 0.0 < float(want[i].mean()) < 0.6, (tag, i, float(want[i].mean()))


@pytest.mark.parametrize("n", [64, 512, 2048])
@pytest.mark.parametrize("mode", ["FULL7", "JACOBIAN"])
def test_kernel_matches_restatement_single_tile(n, mode):
    import watersurfacerendering_amd as W
    b = W.OceanBatch(n, 1, 0)
    b.set_mode(getattr(W._abi, "OCEAN_MODE_" + mode))
    b.prepare(0x5EED0000 + n)
    _run_against_restatement(b, 1, 40, {}, (0.01, 0.30), mode == "JACOBIAN", (n, mode))
    b.close()


@pytest.mark.parametrize("mode", ["FULL7", "JACOBIAN"])
def test_kernel_matches_restatement_batch_of_three_lengths(mode):
    import watersurfacerendering_amd as W
    b = W.OceanBatch(256, 3, 0)
    for i, L in enumerate(LENGTHS3):
        b.set_params(tile=i, tile_length=L)
    b.set_mode(getattr(W._abi, "OCEAN_MODE_" + mode))
    b.prepare(0x5EED0000 + 256)
    _run_against_restatement(b, 3, 40, dict(threshold=0.95), (0.005, 0.60), mode == "JACOBIAN", ("batch", mode))
    b.close()


def test_per_tile_lambdas_reach_the_kernel():
    """FULL7 frames whose tiles differ in lambda: J uses the lambda recorded for each tile's frame."""
    import watersurfacerendering_amd as W
    lambdas = [-1.0, -1.6, -0.7]
    b = W.OceanBatch(128, 3, 0)
    for i, lam in enumerate(lambdas):
        b.set_lambda(lam, i)
    b.prepare(77)
    _run_against_restatement(b, 3, 10, dict(threshold=0.8), (0.0, 1.0), False, "lambdas", lambdas)
    b.close()


def test_pipelined_updates_are_ordered():
    """Depth 3: 12 asynchronous frames with an update behind each and no host synchronisation in between equal a serial context's."""
    import watersurfacerendering_amd as W
    n = 512
    s = W.OceanBatch(n, 1, 0)
    s.prepare(9)
    for j in range(12):
        s.compute_waves(_time(j))
        s.update_foam(DT)
    want = s.read_foam(0)
    s.close()
    assert 0.0 < float(want.mean()) < 0.6
    p = W.OceanBatch(n, 1, 0)
    p.set_pipeline_depth(3)
    p.prepare(9)
    for j in range(12):
        p.compute_waves_async(_time(j))
        p.update_foam(DT)
    got = p.read_foam(0)
    assert np.array_equal(got, want), int((got != want).sum())
    p.close()


def test_update_of_one_tile_leaves_the_others():
    import watersurfacerendering_amd as W
    b = W.OceanBatch(128, 3, 0)
    b.prepare(5)
    b.compute_waves(1.0)
    for _ in range(3):
        b.update_foam(DT, threshold=0.9)
    before = [b.read_foam(i) for i in range(3)]
    assert all(f.mean() > 0 for f in before)
    b.compute_waves(2.0)
    b.update_foam(DT, tile=1, threshold=0.9)
    after = [b.read_foam(i) for i in range(3)]
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])
    assert not np.array_equal(after[1], before[1])
    disp, nrm = b.read_maps()
    p = FM.params(threshold=0.9)
    want = FM.step(before[1], FM.jacobian(disp[1], nrm[1], -1.0, False), p, FM.decay(DT, p["lifetime"]))
    assert np.array_equal(after[1], want)
    b.update_foam(DT, tile=1, threshold=0.9)             # twice behind one frame: two steps
    want = FM.step(want, FM.jacobian(disp[1], nrm[1], -1.0, False), p, FM.decay(DT, p["lifetime"]))
    assert np.array_equal(b.read_foam(1), want) and np.array_equal(b.read_foam(0), before[0])
    b.close()


def test_state_lifetime():
    import watersurfacerendering_amd as W
    A = W._abi
    b = W.OceanBatch(64, 1, 0)
    assert b.device_foam() is None
    b.reset_foam()                                      # nothing allocated yet: nothing to do
    b.prepare(3)
    b.compute_waves(1.0)
    b.update_foam(DT, threshold=0.9)
    first = b.read_foam(0)
    assert first.mean() > 0
    d0 = b.device_foam()
    assert d0
    b.update_foam(DT, threshold=0.9)
    d1 = b.device_foam()
    assert d1 and d1 != d0                              # the two buffers alternate
    b.reset_foam()
    assert not b.read_foam(0).any()                     # zeroed, still ready
    b.update_foam(DT, threshold=0.9)
    assert np.array_equal(b.read_foam(0), first)        # from zero: the first step again
    b.prepare(3)
    with pytest.raises(W.OceanError) as e:
        b.read_foam(0)                                  # Prepare: not ready until the next update
    assert e.value.code == A.OCEAN_E_NOT_READY
    assert b.device_foam() is None
    b.compute_waves(1.0)
    b.update_foam(DT, threshold=0.9)
    assert np.array_equal(b.read_foam(0), first)        # ... and zeroed
    b.set_tile_size(128)                                # frees it
    assert b.device_foam() is None
    b.prepare(3)
    b.compute_waves(1.0)
    b.update_foam(DT, threshold=0.9)
    f = b.read_foam(0)
    assert f.shape == (128, 128) and f.mean() > 0
    disp, nrm = b.read_maps()
    p = FM.params(threshold=0.9)
    assert np.array_equal(f, FM.step(np.zeros((128, 128), np.float32), FM.jacobian(disp[0], nrm[0], -1.0, False), p, FM.decay(DT, p["lifetime"])))
    b.close()


def test_foam_behind_caller_bound_output():
    import torch
    import watersurfacerendering_amd as W
    n = 128

    def run(b):
        b.prepare(21)
        for j in range(6):
            b.compute_waves(_time(j))
            b.update_foam(DT, threshold=0.9)
        return b.read_foam(0)
    ref = W.OceanBatch(n, 1, 0)
    want = run(ref)
    ref.close()
    assert want.mean() > 0
    maps = torch.zeros((2, n, n, 4), dtype=torch.float32, device="cuda")
    b = W.OceanBatch(n, 1, 0)
    b.bind_output(maps[0].data_ptr(), maps[1].data_ptr())
    got = run(b)
    assert np.array_equal(got, want)
    b.synchronize()
    b.bind_output(None, None)
    b.close()


def _points(kind, count, half, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.uniform(-half, half, (count, 2)).astype(np.float32)
    side = int(np.sqrt(count))
    g = (np.arange(side, dtype=np.float32) + 0.5) * np.float32(2 * half / side) - np.float32(half)
    xz = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)
    return (xz + rng.uniform(-0.4, 0.4, xz.shape) * np.float32(2 * half / side)).astype(np.float32)


def _compare_solve(got, want, tag):
    """The rule of tests/test_surface_query_gpu.py::_compare for (r.x, r.z, residual): every point where both residuals are < 1e-3 m agrees
    to 1e-5 of the xz range; a point may go to another root only where the restatement's residual is >= 1e-3 m, and those are < 0.1 %."""
    scale = max(float(np.abs(want[:, 1:3]).max()), 1e-30)
    close = np.all(np.abs(got[:, 1:] - want[:, 1:]) <= 1e-5 * scale, axis=1)
    both = (got[:, 3] < 1e-3) & (want[:, 3] < 1e-3)
    assert close[both].all(), (tag, int((~close & both).sum()))
    other = ~close
    assert not (other & (want[:, 3] < 1e-3)).any(), (tag, int((other & (want[:, 3] < 1e-3)).sum()))
    assert other.sum() < 1e-3 * len(got), (tag, int(other.sum()))
    return int(np.all(got.view(np.uint32) == want.view(np.uint32), axis=1).sum())


@pytest.mark.parametrize("n,cascades", [(64, 1), (64, 3), (512, 1), (512, 3)])
def test_query_matches_restatement(n, cascades):
    import torch
    import watersurfacerendering_amd as W
    lengths = [1000.0] if cascades == 1 else LENGTHS3
    b = W.OceanBatch(n, len(lengths), 0)
    for i, L in enumerate(lengths):
        b.set_params(tile=i, tile_length=L)
    b.prepare(0x5EED0000 + n)
    for j in range(10):
        amps = [float(a) for a in b.compute_waves(_time(j))]
        b.update_foam(DT, threshold=0.95)
    disp, nrm = b.read_maps()
    foams = [b.read_foam(i) for i in range(len(lengths))]
    assert all(0.0 < f.mean() < 1.0 for f in foams)
    grid = 512
    vd = lengths[0] / grid
    scales = [lengths[0] / L for L in lengths]
    for kind in ("random", "grid"):
        xz = _points(kind, 16384, 700.0, seed=n)
        got = b.query_foam(xz, 0, scales, grid, vd, -1.0, 8)
        # out.x against the restated bilinear sample at the RETURNED rest point: every operation correctly rounded, so bit for bit
        sample = FM.sample_foam(foams, scales, grid, vd, got[:, 1], got[:, 2])
        assert np.array_equal(got[:, 0].view(np.uint32), sample.view(np.uint32)), (kind, int((got[:, 0] != sample).sum()))
        assert got[:, 0].max() > 0 and (got[:, 0] > 0).mean() > 0.01
        want = FM.query_foam(foams, list(disp), list(nrm), amps, [-1.0] * len(lengths), lengths, scales, grid, vd, xz, 8)
        same = _compare_solve(got, want, (n, cascades, kind))
        print(f"n={n} cascades={cascades} {kind}: {same}/{len(xz)} points bit-identical, foam > 0 at {(got[:, 0] > 0).mean():.3f}")
        d_xz = torch.from_numpy(xz).cuda()
        d_out = torch.empty((len(xz), 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        b.query_foam_device(d_xz.data_ptr(), len(xz), d_out.data_ptr(), 0, scales, grid, vd, -1.0, 8)
        b.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), got.view(np.uint32))
    b.close()


def test_errors():
    import watersurfacerendering_amd as W
    A = W._abi
    L = A.lib()
    b = W.OceanBatch(64, 2, 0)
    xz = _points("random", 16, 100.0)
    f = b.foam_params()
    buf = np.zeros((64, 64), np.float32)
    with pytest.raises(W.OceanError) as e:
        b.update_foam(DT)                                   # nothing prepared
    assert e.value.code == A.OCEAN_E_NOT_READY
    b.prepare(3)
    with pytest.raises(W.OceanError) as e:
        b.update_foam(DT)                                   # no frame yet
    assert e.value.code == A.OCEAN_E_NOT_READY
    b.compute_waves(1.0)
    for call in (lambda: b.read_foam(0), lambda: b.query_foam(xz)):
        with pytest.raises(W.OceanError) as e:
            call()                                          # no update since Prepare
        assert e.value.code == A.OCEAN_E_NOT_READY
    assert L.ocean_update_foam(b._h, 0, None, DT) == A.OCEAN_E_INVALID
    assert L.ocean_update_foam(b._h, 2, C.byref(f), DT) == A.OCEAN_E_INVALID            # a tile outside the batch
    for kw in (dict(lifetime=0.0), dict(lifetime=-1.0), dict(spread=-0.1), dict(spread=1.5), dict(cutoff=-0.1), dict(cutoff=1.5),
               dict(threshold=float("nan")), dict(gain=float("inf")), dict(lifetime=float("inf")), dict(spread=float("nan")),
               dict(cutoff=float("nan"))):
        with pytest.raises(W.OceanError) as e:
            b.update_foam(DT, **kw)
        assert e.value.code == A.OCEAN_E_INVALID, kw
    for dt in (-0.1, float("nan"), float("inf")):
        with pytest.raises(W.OceanError) as e:
            b.update_foam(dt)
        assert e.value.code == A.OCEAN_E_INVALID, dt
    b.update_foam(0.0)                                      # dt = 0 is a step without decay
    b.update_foam(DT, tile=1)
    assert L.ocean_read_foam(b._h, 0, None) == A.OCEAN_E_INVALID
    assert L.ocean_read_foam(b._h, 2, buf.ctypes.data_as(C.c_void_p)) == A.OCEAN_E_INVALID
    assert L.ocean_device_foam(b._h, None) == A.OCEAN_E_INVALID
    for kw in (dict(uv_scales=(1.0,) * 3), dict(first_tile=2), dict(first_tile=1, uv_scales=(1.0, 1.0)), dict(grid_size=0), dict(iterations=33)):
        with pytest.raises(W.OceanError) as e:
            b.query_foam(xz, **kw)
        assert e.value.code == A.OCEAN_E_INVALID, kw
    s = b._surface(0, (1.0,), None, None, -1.0, 8)
    s.cascades = 0
    assert L.ocean_query_foam(b._h, C.byref(s), None, 0, None) == A.OCEAN_E_INVALID
    s.cascades = 9
    assert L.ocean_query_foam(b._h, C.byref(s), None, 0, None) == A.OCEAN_E_INVALID
    s.cascades = 1
    assert L.ocean_query_foam(b._h, None, None, 0, None) == A.OCEAN_E_INVALID
    assert L.ocean_query_foam(b._h, C.byref(s), None, 4, None) == A.OCEAN_E_INVALID
    assert L.ocean_query_foam_device(b._h, C.byref(s), None, 4, None) == A.OCEAN_E_INVALID
    assert L.ocean_query_foam(b._h, C.byref(s), None, 0, None) == A.OCEAN_OK                # points = 0: nothing to do
    assert L.ocean_query_foam_device(b._h, C.byref(s), None, 0, None) == A.OCEAN_OK
    assert b.query_foam(xz, first_tile=1).shape == (16, 4)
    for mode in (A.OCEAN_MODE_CHOPPY5, A.OCEAN_MODE_HEIGHT1):
        b.set_mode(mode)
        b.compute_waves(1.0)
        with pytest.raises(W.OceanError) as e:
            b.update_foam(DT)                               # the Jacobian's ingredients are not in these maps
        assert e.value.code == A.OCEAN_E_UNSUPPORTED, mode
    b.set_mode(A.OCEAN_MODE_JACOBIAN)                       # the source follows the frame, not the setting: still the HEIGHT1 frame
    with pytest.raises(W.OceanError) as e:
        b.update_foam(DT)
    assert e.value.code == A.OCEAN_E_UNSUPPORTED
    b.compute_waves(1.0)
    b.update_foam(DT)
    b.close()


def test_cpp_adaptor_foam_matches_python_binding(tmp_path):
    import watersurfacerendering_amd as W
    from watersurfacerendering_amd import _abi
    exe = tmp_path / "foam_demo"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "foam_demo.cpp"), "-o", str(exe),
                    "-L", os.path.dirname(_abi.LIB_PATH), "-locean_hip", "-Wl,-rpath," + os.path.dirname(_abi.LIB_PATH),
                    "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = tmp_path / "foam.bin"
    steps = 20
    r = subprocess.run([str(exe), "128", str(out), str(steps)], capture_output=True, text=True, check=True)
    n, _, points, mean = r.stdout.split()
    n, points = int(n), int(points)
    raw = np.fromfile(out, dtype=np.float32)
    cfoam = raw[:n * n].reshape(n, n)
    xz = raw[n * n:n * n + 2 * points].reshape(points, 2)
    cres = raw[n * n + 2 * points:].reshape(points, 4)
    ws = W.WSTessendorf(128, 1000.0)
    ws.SetWindDirection((1.0, 0.5))
    ws.Prepare(seed=42)
    for j in range(steps):
        ws.ComputeWaves(_time(j))
        ws.UpdateFoam(DT)
    foam = ws.GetFoam()
    assert foam.mean() > 0 and float(mean) == pytest.approx(float(foam.mean(dtype=np.float64)), rel=1e-6)
    assert np.array_equal(foam, cfoam)
    assert np.array_equal(ws.QueryFoam(xz).view(np.uint32), cres.view(np.uint32))
