"""float32 numpy restatement of the spray emitters (include/ocean_consumers.h: ocean_emit_spray / _device; the kernels are k_spray_count,
k_spray_scan and k_spray_scatter in watersurfacerendering_amd/csrc/ocean_spray_kernels.h), the cases the CPU and GPU tests share, and the
context that serves the crafted maps of tests/crafted_maps.py to the kernels.  TEST INFRASTRUCTURE ONLY.

A lattice index i of the window is grid vertex (ix0 + i % nx, iy0 + i / nx), evaluated as oracle/consumer.py::displace_grid_cascades
evaluates a vertex (same px, same u, same sampler, same sums); J_c is tests/foam.py's jacobian() of the cascade's two SAMPLES, J their
np.fmin from FLT_MAX in cascade order; V the twins' displacement samples summed as tests/velocity.py::velocity_at sums them, at the vertex's
(u, v); the strength tests/foam.py's generation().  The list is np.flatnonzero of the predicate: ascending i.
"""
import numpy as np

import crafted_maps as CM
import foam as FO
from oracle.consumer import sample_linear_repeat

F = np.float32
CHUNK, SCAN_WIDTH = 1024, 256           # C and the scan width of ocean_spray_kernels.h (SPRAY_CHUNK, SPRAY_SCAN_WIDTH)
DEFAULTS = dict(threshold=0.3, gain=2.5, min_rise=0.0, thin_log2=0, salt=0)
FULL7, CHOPPY5, JACOBIAN = 0, 1, 3      # OCEAN_MODE_*
MODES = (FULL7, JACOBIAN)


def hash32(x):
    """The header's hash on a uint32 array (wraparound)."""
    x = np.array(x, dtype=np.uint32)
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
    return x


def hash32_scalar(x):
    """The same on one Python integer."""
    m = 0xffffffff
    x &= m
    x ^= x >> 16; x = (x * 0x7feb352d) & m; x ^= x >> 15; x = (x * 0x846ca68b) & m; x ^= x >> 16
    return x


def whole_grid(grid):
    return (-(grid // 2), -(grid // 2), grid + 1, grid + 1)


def params(**kw):
    p = dict(DEFAULTS)
    for k in kw:
        if k not in p:
            raise TypeError(k)
    p.update(kw)
    return p


def evaluate(disps, nrms, amps, lambdas, uv_scales, grid, vertex_distance, window, from_slot, twin_disps=None, twin_amps=None):
    """Every vertex of the window: (pos [points, 3], J [points], V [points, 3]); V is zero without twins."""
    ix0, iy0, nx, ny = window
    half = grid // 2
    i = np.arange(nx * ny, dtype=np.int64)
    xi, yi = (ix0 + i % nx).astype(np.int32), (iy0 + i // nx).astype(np.int32)
    px = xi.astype(np.float32) * F(vertex_distance)
    pz = yi.astype(np.float32) * F(vertex_distance)
    u = (xi + np.int32(half)).astype(np.float32) / F(grid)
    v = (yi + np.int32(half)).astype(np.float32) / F(grid)
    dx = np.zeros(nx * ny, np.float32); dy = dx.copy(); dz = dx.copy()
    j = np.full(nx * ny, np.finfo(np.float32).max, np.float32)
    for d, q, amp, lam, sc in zip(disps, nrms, amps, lambdas, uv_scales):
        us, vs = u * F(sc), v * F(sc)
        sd = sample_linear_repeat(np.ascontiguousarray(d, dtype=np.float32), us, vs)
        sl = sample_linear_repeat(np.ascontiguousarray(q, dtype=np.float32), us, vs)
        j = np.fmin(j, FO.jacobian(sd, sl, lam, from_slot))
        dx = dx + sd[:, 0]; dy = dy + sd[:, 1] * F(amp); dz = dz + sd[:, 2]
    pos = np.stack([px + dx, F(0.0) + dy, pz + dz], axis=1).astype(np.float32)
    vel = np.zeros((nx * ny, 3), np.float32)
    if twin_disps is not None:
        vx, vy, vz = np.zeros_like(dx), np.zeros_like(dx), np.zeros_like(dx)
        for d, amp, sc in zip(twin_disps, twin_amps, uv_scales):
            sd = sample_linear_repeat(np.ascontiguousarray(d, dtype=np.float32), u * F(sc), v * F(sc))
            vx = vx + sd[:, 0]; vy = vy + sd[:, 1] * F(amp); vz = vz + sd[:, 2]
        vel = np.stack([vx, vy, vz], axis=1).astype(np.float32)
    return pos, j.astype(np.float32), vel


def predicate(j, vel, twinned, p, points):
    """The three terms of the header's predicate, each [points] bool: (breaking, rising, kept by the thinning)."""
    breaking = j < F(p["threshold"])
    rising = vel[:, 1] >= F(p["min_rise"]) if twinned else np.ones(points, bool)
    h = hash32(np.arange(points, dtype=np.uint32) + np.uint32(p["salt"] & 0xffffffff))
    kept = (h & np.uint32((1 << p["thin_log2"]) - 1)) == 0
    return breaking, rising, kept


def emit(disps, nrms, amps, lambdas, uv_scales, grid, vertex_distance, window, from_slot, twin_disps=None, twin_amps=None, **kw):
    """ocean_emit_spray without a capacity: (pos [total, 4], vel [total, 4], index [total] uint32) -- a capacity keeps the first rows."""
    p = params(**kw)
    points = window[2] * window[3]
    with np.errstate(over="ignore", invalid="ignore"):
        xyz, j, v = evaluate(disps, nrms, amps, lambdas, uv_scales, grid, vertex_distance, window, from_slot, twin_disps, twin_amps)
        breaking, rising, kept = predicate(j, v, twin_disps is not None, p, points)
        index = np.flatnonzero(breaking & rising & kept)
        strength = FO.generation(j, dict(threshold=F(p["threshold"]), gain=F(p["gain"])))
    pos = np.concatenate([xyz, strength[:, None]], axis=1).astype(np.float32)[index]
    vel = np.concatenate([v, j[:, None]], axis=1).astype(np.float32)[index]
    return pos, vel, index.astype(np.uint32)


def chunk_offsets(index, points):
    """The exclusive scan of the passing vertices per chunk of CHUNK lattice indices: what k_spray_scan leaves in the scratch array."""
    counts = np.bincount(np.asarray(index, dtype=np.int64) // CHUNK, minlength=(points + CHUNK - 1) // CHUNK)
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
GRID, VD = 40, 25.0                     # 0.4 texels of tile 0 per vertex: a window of a few hundred vertices crosses many of the 2 x 2 texel blocks
WINDOW = (-20, -12, 41, 25)             # 1025 vertices: one more than C
# (nx * ny, window): around a wave, a 256-thread round, C, and scan width * C + 1; nx != ny throughout; some start at negative vertices
# (half = 20), some beyond the grid
SIZES = ((1, (3, -7, 1, 1)), (63, (-40, 10, 9, 7)), (64, (5, 5, 16, 4)), (65, (-300, -300, 13, 5)), (255, (15, 15, 17, 15)),
         (256, (-8, -8, 32, 8)), (257, (-128, 5, 257, 1)), (CHUNK - 1, (-16, -16, 33, 31)), (CHUNK, (-16, -16, 64, 16)),
         (CHUNK + 1, WINDOW), (SCAN_WIDTH * CHUNK + 1, (-272, -240, 545, 481)))
FAR_WINDOWS = ((-1000, -900, 40, 30), (700, 650, 30, 40))
ODD_GRIDS = (511, 37)                   # whole grids: 512^2 = scan width * C vertices exactly, and 38^2
CASCADE_SETS = ((0, 1), (0, 3), (3, 3), (0, 8))
TWIN_SETS = ((0, 1), (0, 3), (1, 3))    # of the twinned fixture: tiles 4 .. 7 are the twins of 0 .. 3
# J < threshold splits every window of >= C - 1 vertices used below into at least 64 passing and 64 failing vertices (tests/test_spray.py):
# FULL7 gives J of tile 0 from its block values, 1 +- a few percent from the noise of tiles 1 .. 7; JACOBIAN the uniform w of crafted_maps
THRESHOLDS = {(FULL7, 0, 1): 0.3, (FULL7, 0, 3): 0.3, (FULL7, 3, 3): 1.0, (FULL7, 0, 8): 0.3, (FULL7, 1, 3): 1.0,
              (JACOBIAN, 0, 1): 0.3, (JACOBIAN, 0, 3): 0.0, (JACOBIAN, 3, 3): 0.0, (JACOBIAN, 0, 8): -0.3, (JACOBIAN, 1, 3): 0.0}
ALL_PASS, NONE_PASS = 1.0e30, -1.0e30
THIN = dict(thin_log2=3, salt=0x9E3779B9)
MIN_RISE = 0.05


def cases(mode, twinned):
    """(tag, mixed, first, count, uv_scales, grid, vertex_distance, window, params) of one fixture and frame mode.  mixed: the case claims
    at least 64 passing and 64 failing vertices."""
    out = []
    t = lambda first, count: THRESHOLDS[(mode, first, count)]
    if not twinned:
        for points, w in SIZES:
            assert w[2] * w[3] == points and w[2] != w[3] or points == 1
            out.append((f"{points} vertices", points >= CHUNK - 1, 0, 3, CM.scales(0, 3), GRID, VD, w, dict(threshold=t(0, 3))))
        for w in FAR_WINDOWS:
            out.append((f"window at {w[:2]}", True, 0, 3, CM.scales(0, 3), GRID, VD, w, dict(threshold=t(0, 3))))
        for g in ODD_GRIDS:
            out.append((f"grid {g}", True, 0, 3, CM.scales(0, 3), g, 1000.0 / 512.0 if g == 511 else VD, whole_grid(g), dict(threshold=t(0, 3))))
        for first, count in CASCADE_SETS:
            out.append((f"tiles {first}..{first + count - 1}", True, first, count, CM.scales(first, count), GRID, VD, WINDOW, dict(threshold=t(first, count))))
        out.append(("free uv_scales, gain 0.7", True, 0, 3, [1.0, 0.37, 2.7], GRID, VD, WINDOW, dict(threshold=t(0, 3), gain=0.7)))
        out.append(("thinned", False, 0, 3, CM.scales(0, 3), GRID, VD, WINDOW, dict(threshold=ALL_PASS, **THIN)))
        out.append(("all pass", False, 0, 3, CM.scales(0, 3), GRID, VD, WINDOW, dict(threshold=ALL_PASS)))
        out.append(("none pass", False, 0, 3, CM.scales(0, 3), GRID, VD, WINDOW, dict(threshold=NONE_PASS)))
    else:
        for first, count in TWIN_SETS:
            out.append((f"twinned tiles {first}..{first + count - 1}", False, first, count, CM.scales(first, count), GRID, VD, WINDOW,
                        dict(threshold=t(first, count))))
        out.append(("min_rise", False, 0, 3, CM.scales(0, 3), GRID, VD, WINDOW, dict(threshold=ALL_PASS, min_rise=MIN_RISE)))
        out.append(("min_rise, thinned", False, 0, 3, CM.scales(0, 3), GRID, VD, (-272, -240, 545, 481), dict(threshold=t(0, 3), min_rise=-MIN_RISE, **THIN)))
    return out


def restate(disp, nrm, amps, mode, twinned, first, count, uv_scales, grid, vd, window, **kw):
    """emit() on tiles first .. first + count - 1 of the crafted maps with crafted_maps' lambdas; twinned: tile c's twin is tile c + 4."""
    sl = slice(first, first + count)
    tw = slice(first + 4, first + 4 + count)
    return emit(list(disp[sl]), list(nrm[sl]), list(amps[sl]), CM.LAMBDAS[sl], uv_scales, grid, vd, window, mode == JACOBIAN,
                list(disp[tw]) if twinned else None, list(amps[tw]) if twinned else None, **kw)


class Sea:
    """The context behind the GPU tests, in the manner of crafted_maps.Sea: 8 tiles of 16^2 with crafted_maps' lengths and lambdas -- with
    twinned, tiles 4 .. 7 are the twins of 0 .. 3 and run with their sources' -- writing into caller-bound tensors.  frame(mode) runs one
    ordinary frame in that mode (it gives A_c, lambda_c and the recorded mode) and then puts the crafted maps where the kernels read them."""

    def __init__(self, twinned):
        import torch
        import watersurfacerendering_amd as W
        self.twinned = twinned
        self.disp, self.nrm = CM.maps()
        self.bound = torch.zeros((2, CM.TILES, CM.N, CM.N, 4), dtype=torch.float32, device="cuda")
        self.crafted = torch.from_numpy(np.stack([self.disp, self.nrm])).cuda()
        b = self.b = W.OceanBatch(CM.N, CM.TILES, 0)
        b.bind_output(self.bound[0].data_ptr(), self.bound[1].data_ptr())
        if twinned:
            for i in range(4):
                b.set_velocity_twin(4 + i, i)
        for i in range(4 if twinned else CM.TILES):
            b.set_params(tile=i, tile_length=CM.LENGTHS[i], lambda_=CM.LAMBDAS[i])
        b.prepare(0x5EED0000 + CM.N)
        self.mode = None

    def frame(self, mode):
        import torch
        if mode == self.mode:
            return self
        self.b.set_mode(mode)
        self.amps = [float(a) for a in self.b.compute_waves(3.7)]
        assert min(self.amps) > 0.0
        self.b.synchronize()
        self.bound.copy_(self.crafted)
        torch.cuda.synchronize()
        self.mode = mode
        return self

    def restate(self, first, count, uv_scales, grid, vd, window, **kw):
        return restate(self.disp, self.nrm, self.amps, self.mode, self.twinned, first, count, uv_scales, grid, vd, window, **kw)

    def close(self):
        self.b.synchronize()
        self.b.bind_output(None, None)
        self.b.close()
