"""watersurfacerendering_amd -- MI355X-native Tessendorf FFT ocean synthesiser.

Host-side mirror of the reference's `class WSTessendorf`
(/root/reference/src/scene/WSTessendorf.h:58-122) over the C ABI of
include/ocean.h (libocean_hip.so: hand-written HIP for gfx950).  Same method
names, argument meaning and (absence of) error behaviour as the reference class
so parity tests read like calls on the original object:

    ws = WSTessendorf(512, 1000.0)
    ws.SetWindDirection((1.0, 0.0)); ws.SetWindSpeed(10.0)
    ws.Prepare(seed=7)
    A = ws.ComputeWaves(1.5)
    disp, normals = ws.GetDisplacements(), ws.GetNormals()     # (N, N, 4) float32

`OceanBatch` exposes the batched / asynchronous surface (T independent tiles
per context, device-resident maps, event timing) the bench and the multi-GPU
path use.  Nothing here falls back to a CPU implementation.
"""
from __future__ import annotations

import ctypes as C
import math

from typing import Optional

import numpy as np

from . import _abi
from ._abi import OceanError, Params, build  # noqa: F401

__all__ = ["WSTessendorf", "OceanBatch", "OceanError", "build", "host_register", "host_unregister", "comm_unique_id", "BODY_DTYPE", "WAVE_DTYPE",
           "sky_params", "water_params", "sky_coefficients"]

#: struct ocean_body (include/ocean_consumers.h) as a numpy record: what OceanBatch.buoyancy takes
BODY_DTYPE = np.dtype([("pos", np.float32, 3), ("quat", np.float32, 4), ("vel", np.float32, 3), ("omega", np.float32, 3),
                       ("first_point", np.uint32), ("points", np.uint32), ("reserved", np.uint32)])

#: struct ocean_wave (include/ocean_consumers.h) as a numpy record: what OceanBatch.extract_waves returns and set_waves takes
WAVE_DTYPE = np.dtype([("jx", np.int32), ("jz", np.int32), ("kx", np.float32), ("kz", np.float32), ("ux", np.float32), ("uz", np.float32),
                       ("re", np.float32), ("im", np.float32), ("omega", np.float32), ("bin", np.uint32), ("reserved", np.float32, 2)])


def _dev_ptr(x):
    """A device array as the C ABI takes it: a torch tensor's data_ptr(), an integer address, or None."""
    if x is None:
        return None
    return C.c_void_p(int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x))


def _patched(struct, fields):
    for k, v in fields.items():
        kind = dict(struct._fields_).get(k)
        if kind is None:
            raise TypeError(f"unknown field {k!r} of {type(struct).__name__}")
        if kind is C.c_uint32:
            setattr(struct, k, int(v))
        elif kind is C.c_float:
            setattr(struct, k, float(v))
        else:
            setattr(struct, k, kind(*[float(x) for x in v]))
    return struct


def sky_params(**fields) -> "_abi.Sky":
    """struct ocean_sky with the reference's defaults (ocean_default_sky), patched by sun_dir / turbidity / sun_color / sun_intensity."""
    s = _abi.Sky()
    _abi.lib().ocean_default_sky(C.byref(s))
    return _patched(s, fields)


def water_params(**fields) -> "_abi.Water":
    """struct ocean_water with the reference's defaults (ocean_default_water), patched by any of its fields (cam_pos, height, absorb,
    scatter, backscatter, terrain_color, sky_intensity, specular_intensity, specular_highlights, fresnel, seabed, seabed_factor,
    foam_white, tonemap)."""
    w = _abi.Water()
    _abi.lib().ocean_default_water(C.byref(w))
    return _patched(w, fields)


def sky_coefficients(sky=None) -> "_abi.SkyCoeffs":
    """SkyPreetham::Update on the host (ocean_sky_coefficients): the normalised sun, the turbidity and A, B, C, D, E, ZenithLum,
    ZeroThetaSun in the layout of the reference's uniform block.  Needs neither a context nor a device."""
    k = _abi.SkyCoeffs()
    s = sky_params() if sky is None else sky
    _abi.check(_abi.lib().ocean_sky_coefficients(C.byref(s), C.byref(k)), "ocean_sky_coefficients")
    return k


def _is_pow2(n: int) -> bool:
    return n > 0 and (n & (n - 1)) == 0


class OceanBatch:
    """T independent N x N tiles on one device (ocean_create ... ocean_destroy)."""

    def __init__(self, tile_size: int = 512, tiles: int = 1, device: int = 0):
        self._L = _abi.lib()
        self._h = C.c_void_p()
        _abi.check(self._L.ocean_create(C.byref(self._h), tile_size, tiles, device), "ocean_create")
        self.tiles = tiles
        self.device = device
        self._spectra = {}     # tile -> struct ocean_spectrum as set_spectrum last set it
        self._twins = {}       # twin -> source, as ocean_set_velocity_twin accepted them (what set_params(ALL_TILES) skips)

    # -- lifetime ---------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.ocean_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- properties ---------------------------------------------------------------
    @property
    def tile_size(self) -> int:
        return int(self._L.ocean_tile_size(self._h))

    def get_params(self, tile: int = 0) -> Params:
        p = Params()
        _abi.check(self._L.ocean_get_params(self._h, tile, C.byref(p)), "ocean_get_params")
        return p

    def set_params(self, tile: int = _abi.OCEAN_ALL_TILES, **kw):
        """Patch the given fields of one tile, or of EVERY tile (each keeps its other parameters)."""
        tiles = [i for i in range(self.tiles) if i not in self._twins] if tile == _abi.OCEAN_ALL_TILES else (tile,)   # (a twin has its source's)
        for i in tiles:
            p = self.get_params(i)
            for k, v in kw.items():
                k = "lambda_" if k in ("lambda", "lam") else k
                if not hasattr(p, k):
                    raise TypeError(f"unknown ocean parameter {k!r}")
                setattr(p, k, v)
            _abi.check(self._L.ocean_set_params(self._h, i, C.byref(p)), "ocean_set_params")

    def set_lambda(self, lam: float, tile: int = _abi.OCEAN_ALL_TILES):
        _abi.check(self._L.ocean_set_lambda(self._h, tile, lam), "ocean_set_lambda")

    def set_velocity_twin(self, tile: int, source: Optional[int]):
        """Make `tile` the derivative twin of `source` from the next prepare() on (ocean_set_velocity_twin): its maps then hold the time
        derivative of its source's -- what query_velocity and buoyancy_flow read.  source None makes it an ordinary tile again.  The context
        is not prepared until the next prepare()."""
        src = _abi.OCEAN_NO_SOURCE if source is None else int(source)
        _abi.check(self._L.ocean_set_velocity_twin(self._h, int(tile), src), "ocean_set_velocity_twin")
        if source is None:
            self._twins.pop(int(tile), None)
        else:
            self._twins[int(tile)] = int(source)

    def velocity_twin(self, tile: int) -> Optional[int]:
        """The source `tile` is the twin of, None for an ordinary tile (ocean_velocity_twin)."""
        src = C.c_uint32()
        _abi.check(self._L.ocean_velocity_twin(self._h, int(tile), C.byref(src)), "ocean_velocity_twin")
        return None if src.value == _abi.OCEAN_NO_SOURCE else int(src.value)

    # -- empirical spectra (include/ocean_consumers.h: ocean_set_spectrum) ---------------------------------------------------
    def set_spectrum(self, tile: int = _abi.OCEAN_ALL_TILES, **fields):
        """Patch the given fields of struct ocean_spectrum -- kind, spreading, fetch, gamma, depth, spread_s, swell, alpha, peak_omega,
        k_min, k_max, scale -- of one tile, or of every tile that is not a twin (ocean_set_spectrum); in effect from the next prepare().
        The fields patched are the ones last SET here (alpha / peak_omega 0 = derive stay 0), not the resolved values spectrum() reports."""
        tiles = [i for i in range(self.tiles) if i not in self._twins] if tile == _abi.OCEAN_ALL_TILES else (int(tile),)
        for i in tiles:
            s = _abi.Spectrum()
            C.memmove(C.byref(s), C.byref(self._spectra[i]), C.sizeof(s)) if i in self._spectra else self._L.ocean_default_spectrum(C.byref(s))
            for k, v in fields.items():
                if k not in dict(_abi.Spectrum._fields_):
                    raise TypeError(f"unknown spectrum field {k!r}")
                setattr(s, k, int(v) if k in ("kind", "spreading") else float(v))
            _abi.check(self._L.ocean_set_spectrum(self._h, i, C.byref(s)), "ocean_set_spectrum")
            self._spectra[i] = s

    def spectrum(self, tile: int = 0) -> "_abi.Spectrum":
        """struct ocean_spectrum of `tile` (a twin: its source's), alpha / peak_omega as the last prepare() resolved them (ocean_get_spectrum)."""
        s = _abi.Spectrum()
        _abi.check(self._L.ocean_get_spectrum(self._h, int(tile), C.byref(s)), "ocean_get_spectrum")
        return s

    def spectrum_moments(self, tile: int = 0) -> np.ndarray:
        """(sum |h0|^2, sum k |h0|^2, sum k^2 |h0|^2) of the tile's prepared spectrum as float64 (ocean_spectrum_moments): the height
        variance m0 in m^2 -- Hs = 4 sqrt(m0) --, the first moment, the mean-square slope.  Synchronises."""
        out = (C.c_double * 3)()
        _abi.check(self._L.ocean_spectrum_moments(self._h, int(tile), out), "ocean_spectrum_moments")
        return np.array(out[:], dtype=np.float64)

    def set_tile_size(self, n: int):
        _abi.check(self._L.ocean_set_tile_size(self._h, n), "ocean_set_tile_size")

    # -- Prepare / ComputeWaves -----------------------------------------------------
    def prepare(self, seed: int = 0, xi: np.ndarray | None = None):
        ptr = None
        if xi is not None:
            n = self.tile_size
            xi = np.ascontiguousarray(xi, dtype=np.float32).reshape(self.tiles, n, n, 2)
            ptr = xi.ctypes.data_as(C.c_void_p)
        _abi.check(self._L.ocean_prepare(self._h, seed & 0xFFFFFFFFFFFFFFFF, ptr), "ocean_prepare")

    def compute_waves(self, t: float) -> np.ndarray:
        amp = np.empty(self.tiles, dtype=np.float32)
        _abi.check(self._L.ocean_compute_waves(self._h, t, amp.ctypes.data_as(C.POINTER(C.c_float))),
                   "ocean_compute_waves")
        return amp

    def compute_waves_read(self, t: float, disp: np.ndarray | None = None, nrm: np.ndarray | None = None):
        """ComputeWaves(t) and the read-out of every tile's maps as ONE blocking call (ocean_compute_waves_read: the normal map's copy
        runs beside the displacement pass).  Returns (amplitudes, disp, nrm); disp / nrm [tiles, N, N, 4] float32 are allocated unless
        passed in (pass page-locked arrays -- host_register -- for true DMAs)."""
        n = self.tile_size
        amp = np.empty(self.tiles, dtype=np.float32)
        d = np.empty((self.tiles, n, n, 4), dtype=np.float32) if disp is None else disp
        q = np.empty((self.tiles, n, n, 4), dtype=np.float32) if nrm is None else nrm
        assert d.dtype == np.float32 and q.dtype == np.float32 and d.size == q.size == self.tiles * n * n * 4 and d.flags.c_contiguous and q.flags.c_contiguous
        _abi.check(self._L.ocean_compute_waves_read(self._h, t, amp.ctypes.data_as(C.POINTER(C.c_float)), d.ctypes.data_as(C.c_void_p),
                                                    q.ctypes.data_as(C.c_void_p)), "ocean_compute_waves_read")
        return amp, d, q

    def set_placement_search(self, trials: int):
        """Candidates the next prepare() times for the spectrum + intermediates (ocean_set_placement_search): 0 = the library's rule, 1 = off."""
        _abi.check(self._L.ocean_set_placement_search(self._h, int(trials)), "ocean_set_placement_search")

    def placement_report(self):
        """(candidates timed by the most recent prepare(), serial frame us of the chosen one, of the slowest one)."""
        n, a, b = C.c_int(), C.c_float(), C.c_float()
        _abi.check(self._L.ocean_placement_report(self._h, C.byref(n), C.byref(a), C.byref(b)), "ocean_placement_report")
        return n.value, a.value, b.value

    @property
    def fault_recoveries(self) -> int:
        """How often the host re-ran frames because an in-launch wait had given up (ocean_fault_recoveries; 0 on a dedicated device)."""
        return int(self._L.ocean_fault_recoveries(self._h))

    def compute_waves_async(self, t: float):
        _abi.check(self._L.ocean_compute_waves_async(self._h, t), "ocean_compute_waves_async")

    def wait_frame(self) -> np.ndarray:
        """Amplitudes of the most recently enqueued frame once its last workgroup has finished (ocean_wait_frame: a poll of the
        frame's completion records, not a stream synchronisation; copies enqueued behind the frame may still be running)."""
        amp = np.empty(self.tiles, dtype=np.float32)
        _abi.check(self._L.ocean_wait_frame(self._h, amp.ctypes.data_as(C.POINTER(C.c_float))), "ocean_wait_frame")
        return amp

    def set_frame_tracking(self, on: bool):
        """Asynchronous frames leave completion records too, so that wait_frame() polls instead of synchronising the stream."""
        _abi.check(self._L.ocean_set_frame_tracking(self._h, int(bool(on))), "ocean_set_frame_tracking")

    def set_time_offsets(self, offsets):
        if offsets is None:
            _abi.check(self._L.ocean_set_time_offsets(self._h, None), "ocean_set_time_offsets")
            return
        o = np.ascontiguousarray(offsets, dtype=np.float32)
        assert o.size == self.tiles
        _abi.check(self._L.ocean_set_time_offsets(self._h, o.ctypes.data_as(C.c_void_p)), "ocean_set_time_offsets")

    def synchronize(self):
        _abi.check(self._L.ocean_synchronize(self._h), "ocean_synchronize")

    def heights(self, tile: int = 0):
        a, mn, mx = C.c_float(), C.c_float(), C.c_float()
        _abi.check(self._L.ocean_get_heights(self._h, tile, C.byref(a), C.byref(mn), C.byref(mx)),
                   "ocean_get_heights")
        return a.value, mn.value, mx.value

    # -- read-out -------------------------------------------------------------------
    def read_maps(self, first: int = 0, count: int | None = None):
        count = self.tiles - first if count is None else count
        n = self.tile_size
        d = np.empty((count, n, n, 4), dtype=np.float32)
        q = np.empty((count, n, n, 4), dtype=np.float32)
        _abi.check(self._L.ocean_read_maps(self._h, first, count, d.ctypes.data_as(C.c_void_p),
                                           q.ctypes.data_as(C.c_void_p)), "ocean_read_maps")
        return d, q

    def read_maps_async(self, disp: np.ndarray, nrm: np.ndarray, first: int = 0, count: int | None = None):
        """Enqueue the D2H copy of the last enqueued frame's maps into caller arrays (pin them with
        host_register for a true asynchronous DMA); valid after synchronize()."""
        count = self.tiles - first if count is None else count
        need = count * self.tile_size * self.tile_size * 16           # (the library sees raw pointers: it cannot check the arrays)
        if disp.nbytes < need or nrm.nbytes < need:
            raise ValueError(f"read_maps_async: {count} tile(s) need {need} bytes per array, got {disp.nbytes} and {nrm.nbytes}")
        _abi.check(self._L.ocean_read_maps_async(self._h, first, count, disp.ctypes.data_as(C.c_void_p),
                                                 nrm.ctypes.data_as(C.c_void_p)), "ocean_read_maps_async")

    def read_maps_staging(self, staging: np.ndarray, vertices_bytes: int, indices_bytes: int, tile: int = 0) -> int:
        """The reference's staging upload (WaterSurfaceMesh.cpp:701-755): enqueue the copy of the last enqueued
        frame's maps of `tile` into a byte buffer laid out [vertices | indices | pad16 | displacements | normals].
        Returns the number of bytes the caller then flushes; valid after synchronize()."""
        assert staging.dtype == np.uint8 and staging.flags["C_CONTIGUOUS"]
        n = self.tile_size
        off = int(self._L.ocean_staging_map_offset(vertices_bytes, indices_bytes))
        if staging.nbytes < off + 2 * n * n * 16:
            raise ValueError("staging buffer too small")
        flush = C.c_size_t()
        _abi.check(self._L.ocean_read_maps_staging(self._h, tile, staging.ctypes.data_as(C.c_void_p), vertices_bytes,
                                                   indices_bytes, C.byref(flush)), "ocean_read_maps_staging")
        return int(flush.value)

    # -- multi-GPU gather of the packed maps (RCCL) ------------------------------------------
    def comm_init(self, nranks: int, rank: int, unique_id: bytes):
        assert len(unique_id) == _abi.OCEAN_COMM_ID_BYTES
        buf = C.create_string_buffer(unique_id, _abi.OCEAN_COMM_ID_BYTES)
        _abi.check(self._L.ocean_comm_init(self._h, nranks, rank, buf), "ocean_comm_init")

    def comm_count(self):
        """(ranks, rank) of the context's communicator as RCCL reports them."""
        n, r = C.c_int(), C.c_int()
        _abi.check(self._L.ocean_comm_count(self._h, C.byref(n), C.byref(r)), "ocean_comm_count")
        return n.value, r.value

    def comm_destroy(self):
        _abi.check(self._L.ocean_comm_destroy(self._h), "ocean_comm_destroy")

    def gather_maps(self, root: int, recv_disp: int | None, recv_nrm: int | None, half: bool = False):
        """Enqueue the RCCL gather of the last enqueued frame's maps to `root` (device pointers of the receive
        arrays [nranks][tiles][N][N][4] on the root, None elsewhere); asynchronous, see ocean.h.  half=True sends
        the maps as IEEE halves (receive arrays of float16)."""
        fn = self._L.ocean_gather_maps_f16 if half else self._L.ocean_gather_maps
        _abi.check(fn(self._h, root, C.c_void_p(recv_disp), C.c_void_p(recv_nrm)), "ocean_gather_maps")

    def device_maps(self):
        d, q = C.c_void_p(), C.c_void_p()
        _abi.check(self._L.ocean_device_maps(self._h, C.byref(d), C.byref(q)), "ocean_device_maps")
        return d.value, q.value

    def displace_grid(self, tile: int = 0, grid_size: Optional[int] = None, vertex_distance: Optional[float] = None,
                      uv_scale: float = 1.0, choppy: float = -1.0):
        """Vertex-stage consumer (WaterSurfaceMesh.vert:24-41 on the grid of WaterSurfaceMesh.cpp:500-533) of the
        most recent frame: returns (positions, normals), each ((grid_size+1)^2, 4) float32.  Defaults are the
        reference's: grid_size = tile size, vertex_distance = 1000/512 (WaterSurfaceMesh.h:199-202), choppy =
        the default lambda."""
        g = self.tile_size if grid_size is None else int(grid_size)
        vd = (1000.0 / 512.0) if vertex_distance is None else float(vertex_distance)
        _abi.check(self._L.ocean_displace_grid(self._h, tile, g, vd, uv_scale, choppy), "ocean_displace_grid")
        pos = np.empty(((g + 1) * (g + 1), 4), dtype=np.float32)
        nrm = np.empty_like(pos)
        _abi.check(self._L.ocean_read_grid(self._h, pos.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p)),
                   "ocean_read_grid")
        return pos, nrm

    def displace_grid_cascades(self, uv_scales, first_tile: int = 0, grid_size: Optional[int] = None,
                               vertex_distance: Optional[float] = None, choppy: float = -1.0):
        """Sum of the tiles first_tile .. first_tile+len(uv_scales)-1 as cascades (ocean_displace_grid_cascades):
        returns (positions, normals) like displace_grid."""
        sc = np.ascontiguousarray(uv_scales, dtype=np.float32)
        g = self.tile_size if grid_size is None else int(grid_size)
        vd = (1000.0 / 512.0) if vertex_distance is None else float(vertex_distance)
        _abi.check(self._L.ocean_displace_grid_cascades(self._h, first_tile, sc.size, g, vd, sc.ctypes.data_as(C.POINTER(C.c_float)), choppy),
                   "ocean_displace_grid_cascades")
        pos = np.empty(((g + 1) * (g + 1), 4), dtype=np.float32)
        nrm = np.empty_like(pos)
        _abi.check(self._L.ocean_read_grid(self._h, pos.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p)), "ocean_read_grid")
        return pos, nrm

    def _surface(self, first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations) -> "_abi.Surface":
        sc = [float(x) for x in np.atleast_1d(np.asarray(uv_scales, dtype=np.float32))]
        if not 1 <= len(sc) <= 8:
            raise ValueError("uv_scales: 1 .. 8 cascades")
        s = _abi.Surface()
        s.first_tile, s.cascades = int(first_tile), len(sc)
        s.grid_size = self.tile_size if grid_size is None else int(grid_size)
        s.vertex_distance = (1000.0 / 512.0) if vertex_distance is None else float(vertex_distance)
        s.choppy, s.iterations = float(choppy), int(iterations)
        for i, x in enumerate(sc):
            s.uv_scales[i] = x
        return s

    def query_surface(self, xz, first_tile: int = 0, uv_scales=(1.0,), grid_size: Optional[int] = None,
                      vertex_distance: Optional[float] = None, choppy: float = -1.0, iterations: int = 8):
        """Surface query (ocean_query_surface) on the most recent frame: the displaced position and normal of the surface the
        vertex stage draws (tiles first_tile .. first_tile+len(uv_scales)-1 as cascades) above each world point xz [points, 2].
        Returns (pos, nrm), each (points, 4) float32: pos = (x, height, z, smallest Jacobian slot), nrm = (unit normal, residual
        |P.xz - xz| in metres).  Defaults as displace_grid."""
        q = np.ascontiguousarray(xz, dtype=np.float32).reshape(-1, 2)
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        pos = np.empty((q.shape[0], 4), dtype=np.float32)
        nrm = np.empty_like(pos)
        _abi.check(self._L.ocean_query_surface(self._h, C.byref(s), q.ctypes.data_as(C.c_void_p), q.shape[0],
                                               pos.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p)), "ocean_query_surface")
        return pos, nrm

    def query_surface_device(self, d_xz: int, points: int, d_pos: int, d_nrm: int, first_tile: int = 0, uv_scales=(1.0,),
                             grid_size: Optional[int] = None, vertex_distance: Optional[float] = None, choppy: float = -1.0,
                             iterations: int = 8):
        """query_surface on device arrays of the context's device (ocean_query_surface_device; e.g. torch tensors' data_ptr()):
        d_xz [points][2], d_pos / d_nrm [points][4] float32.  Enqueued on the frame's stream (`stream`); returns at once."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        _abi.check(self._L.ocean_query_surface_device(self._h, C.byref(s), C.c_void_p(d_xz), int(points), C.c_void_p(d_pos),
                                                      C.c_void_p(d_nrm)), "ocean_query_surface_device")

    @staticmethod
    def _raycast(max_distance, steps, refine) -> "_abi.Raycast":
        r = _abi.Raycast()
        r.max_distance, r.steps, r.refine = float(max_distance), int(steps), int(refine)
        return r

    def raycast_surface(self, origins, directions, max_distance: float, steps: int = 0, refine: int = 0, first_tile: int = 0,
                        uv_scales=(1.0,), grid_size: Optional[int] = None, vertex_distance: Optional[float] = None,
                        choppy: float = -1.0, iterations: int = 8):
        """Ray cast (ocean_raycast_surface) on the most recent frame: where each ray origins[i] + t * directions[i] (both [rays, 3];
        directions need not be unit length) first meets the surface query_surface defines, for t in [0, max_distance] metres.
        steps (0 = 64) coarse samples over the part of the ray inside the height slab, refine (0 = 3) rounds of 16-part splits.
        Returns (hit, nrm), each (rays, 4) float32: a hit is (x, height, z, t) and (unit normal, signed gap); an origin under water
        gives (x, height, z, -2) and (unit normal, depth <= 0) at the origin's xz; a miss (0, 0, 0, -1) and zeros."""
        o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError("origins and directions: the same number of rays")
        rays = np.ascontiguousarray(np.concatenate([o, d], axis=1))
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        r = self._raycast(max_distance, steps, refine)
        hit = np.empty((rays.shape[0], 4), dtype=np.float32)
        nrm = np.empty_like(hit)
        _abi.check(self._L.ocean_raycast_surface(self._h, C.byref(s), C.byref(r), rays.ctypes.data_as(C.c_void_p), rays.shape[0],
                                                 hit.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p)), "ocean_raycast_surface")
        return hit, nrm

    def raycast_surface_device(self, d_rays: int, count: int, d_hit: int, d_nrm: int, max_distance: float, steps: int = 0,
                               refine: int = 0, first_tile: int = 0, uv_scales=(1.0,), grid_size: Optional[int] = None,
                               vertex_distance: Optional[float] = None, choppy: float = -1.0, iterations: int = 8):
        """raycast_surface on device arrays of the context's device (ocean_raycast_surface_device; e.g. torch tensors' data_ptr()):
        d_rays [count][6] (ox, oy, oz, dx, dy, dz), d_hit / d_nrm [count][4] float32.  Enqueued on the frame's stream (`stream`);
        returns at once."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        r = self._raycast(max_distance, steps, refine)
        _abi.check(self._L.ocean_raycast_surface_device(self._h, C.byref(s), C.byref(r), C.c_void_p(d_rays), int(count),
                                                        C.c_void_p(d_hit), C.c_void_p(d_nrm)), "ocean_raycast_surface_device")

    # -- persistent foam (include/ocean_consumers.h: ocean_update_foam ...) ---------------------------------------------
    @staticmethod
    def foam_params(**params) -> "_abi.Foam":
        """struct ocean_foam with the library's defaults (ocean_default_foam), patched by threshold / gain / lifetime / spread / cutoff."""
        f = _abi.Foam()
        _abi.lib().ocean_default_foam(C.byref(f))
        for k, v in params.items():
            if k not in ("threshold", "gain", "lifetime", "spread", "cutoff"):
                raise TypeError(f"unknown foam parameter {k!r}")
            setattr(f, k, float(v))
        return f

    def update_foam(self, dt: float, tile: int = _abi.OCEAN_ALL_TILES, **params):
        """One foam step of dt seconds behind the most recent frame (ocean_update_foam), for one tile or all of them: generated where the
        frame's Jacobian is under `threshold`, blended towards the 3 x 3 binomial by `spread`, faded with `lifetime`.  Enqueued; returns at once."""
        f = self.foam_params(**params)
        _abi.check(self._L.ocean_update_foam(self._h, tile, C.byref(f), dt), "ocean_update_foam")

    def reset_foam(self):
        _abi.check(self._L.ocean_reset_foam(self._h), "ocean_reset_foam")

    def read_foam(self, tile: int = 0) -> np.ndarray:
        """Foam coverage of `tile` after the most recent update: (N, N) float32 in [0, 1], in the maps' texel layout (synchronises)."""
        n = self.tile_size
        out = np.empty((n, n), dtype=np.float32)
        _abi.check(self._L.ocean_read_foam(self._h, tile, out.ctypes.data_as(C.c_void_p)), "ocean_read_foam")
        return out

    def device_foam(self) -> Optional[int]:
        """Device address of the foam [tiles][N][N] after the most recently enqueued update (ask again after each update), None before any."""
        p = C.c_void_p()
        _abi.check(self._L.ocean_device_foam(self._h, C.byref(p)), "ocean_device_foam")
        return p.value

    def query_foam(self, xz, first_tile: int = 0, uv_scales=(1.0,), grid_size: Optional[int] = None,
                   vertex_distance: Optional[float] = None, choppy: float = -1.0, iterations: int = 8):
        """Foam above each world point xz [points, 2] (ocean_query_foam), on the surface query_surface defines: returns (points, 4)
        float32 rows (foam, rest x, rest z, residual |P(rest).xz - xz| in metres); foam is the largest of the cascades' samples."""
        q = np.ascontiguousarray(xz, dtype=np.float32).reshape(-1, 2)
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        out = np.empty((q.shape[0], 4), dtype=np.float32)
        _abi.check(self._L.ocean_query_foam(self._h, C.byref(s), q.ctypes.data_as(C.c_void_p), q.shape[0],
                                            out.ctypes.data_as(C.c_void_p)), "ocean_query_foam")
        return out

    def query_foam_device(self, d_xz: int, points: int, d_out: int, first_tile: int = 0, uv_scales=(1.0,),
                          grid_size: Optional[int] = None, vertex_distance: Optional[float] = None, choppy: float = -1.0,
                          iterations: int = 8):
        """query_foam on device arrays of the context's device (ocean_query_foam_device): d_xz [points][2], d_out [points][4] float32.
        Enqueued on the frame's stream (`stream`); returns at once."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        _abi.check(self._L.ocean_query_foam_device(self._h, C.byref(s), C.c_void_p(d_xz), int(points), C.c_void_p(d_out)),
                   "ocean_query_foam_device")

    # -- buoyancy (include/ocean_consumers.h: ocean_set_hull, ocean_buoyancy_bodies) ---------------------------------------
    def set_hull(self, points):
        """Upload the hull sample points [count, 4] (local x, y, z, edge of the cubic cell) the bodies of buoyancy() refer to
        (ocean_set_hull); None or an empty array drops the hull.  Kept across prepare() and set_tile_size()."""
        p = np.zeros((0, 4), np.float32) if points is None else np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
        _abi.check(self._L.ocean_set_hull(self._h, p.ctypes.data_as(C.c_void_p) if len(p) else None, len(p)), "ocean_set_hull")

    @staticmethod
    def buoyancy_params(**params) -> "_abi.Buoyancy":
        """struct ocean_buoyancy with the library's defaults (ocean_default_buoyancy), patched by density / gravity / drag."""
        p = _abi.Buoyancy()
        _abi.lib().ocean_default_buoyancy(C.byref(p))
        for k, v in params.items():
            if k not in ("density", "gravity", "drag"):
                raise TypeError(f"unknown buoyancy parameter {k!r}")
            setattr(p, k, float(v))
        return p

    @staticmethod
    def _body_words(bodies) -> np.ndarray:
        """[count, 16] uint32 words of ocean_body from a BODY_DTYPE record array, or from [count, 16] 4-byte words taken as they are."""
        b = np.asarray(bodies)
        if b.dtype == BODY_DTYPE:
            return np.ascontiguousarray(b).reshape(-1).view(np.uint32).reshape(-1, 16)
        if b.dtype.itemsize != 4 or b.dtype.kind not in "fiu" or b.ndim != 2 or b.shape[1] != 16:
            raise ValueError("bodies: a BODY_DTYPE record array or [count, 16] 4-byte words")
        return np.ascontiguousarray(b).view(np.uint32)

    def buoyancy(self, bodies, first_tile: int = 0, uv_scales=(1.0,), grid_size: Optional[int] = None,
                 vertex_distance: Optional[float] = None, choppy: float = -1.0, iterations: int = 8, **params):
        """Net buoyancy and drag on floating bodies (ocean_buoyancy_bodies) on the most recent frame, over the hull of set_hull():
        bodies is a BODY_DTYPE record array (or [count, 16] words), params patch density / gravity / drag.  Returns (force, torque),
        each (count, 4) float32: force = (F.x, F.y, F.z, submerged volume in m^3), torque = (T about the body origin, the largest
        query residual in metres).  The surface is query_surface's, same defaults."""
        w = self._body_words(bodies)
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        p = self.buoyancy_params(**params)
        force = np.empty((w.shape[0], 4), dtype=np.float32)
        torque = np.empty_like(force)
        _abi.check(self._L.ocean_buoyancy_bodies(self._h, C.byref(s), C.byref(p), w.ctypes.data_as(C.c_void_p), w.shape[0],
                                                 force.ctypes.data_as(C.c_void_p), torque.ctypes.data_as(C.c_void_p)), "ocean_buoyancy_bodies")
        return force, torque

    def buoyancy_device(self, d_bodies: int, count: int, d_force: int, d_torque: int, first_tile: int = 0, uv_scales=(1.0,),
                        grid_size: Optional[int] = None, vertex_distance: Optional[float] = None, choppy: float = -1.0,
                        iterations: int = 8, **params):
        """buoyancy on device arrays of the context's device (ocean_buoyancy_bodies_device; e.g. torch tensors' data_ptr(), 16-byte
        aligned): d_bodies [count][16] words, d_force / d_torque [count][4] float32.  A range that leaves the hull is clamped to it.
        Enqueued on the frame's stream (`stream`); returns at once."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        p = self.buoyancy_params(**params)
        _abi.check(self._L.ocean_buoyancy_bodies_device(self._h, C.byref(s), C.byref(p), C.c_void_p(d_bodies), int(count),
                                                        C.c_void_p(d_force), C.c_void_p(d_torque)), "ocean_buoyancy_bodies_device")

    # -- water velocity (include/ocean_consumers.h: ocean_query_velocity, ocean_buoyancy_bodies_flow) ---------------------------
    def query_velocity(self, xz, first_tile: int = 0, uv_scales=(1.0,), grid_size: Optional[int] = None,
                       vertex_distance: Optional[float] = None, choppy: float = -1.0, iterations: int = 8):
        """Velocity of the water particle at each world point xz [points, 2] (ocean_query_velocity) on the most recent frame.  The tiles
        first_tile .. first_tile+len(uv_scales)-1 are the sources; their twins (set_velocity_twin) must be consecutive tiles in the same
        order.  Returns (pos, vel), each (points, 4) float32: pos exactly as query_surface, vel = (V.x, V.y, V.z in m/s, residual in metres)."""
        q = np.ascontiguousarray(xz, dtype=np.float32).reshape(-1, 2)
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        pos = np.empty((q.shape[0], 4), dtype=np.float32)
        vel = np.empty_like(pos)
        _abi.check(self._L.ocean_query_velocity(self._h, C.byref(s), q.ctypes.data_as(C.c_void_p), q.shape[0],
                                                pos.ctypes.data_as(C.c_void_p), vel.ctypes.data_as(C.c_void_p)), "ocean_query_velocity")
        return pos, vel

    def query_velocity_device(self, d_xz: int, points: int, d_pos: int, d_vel: int, first_tile: int = 0, uv_scales=(1.0,),
                              grid_size: Optional[int] = None, vertex_distance: Optional[float] = None, choppy: float = -1.0,
                              iterations: int = 8):
        """query_velocity on device arrays of the context's device (ocean_query_velocity_device): d_xz [points][2], d_pos / d_vel
        [points][4] float32.  Enqueued on the frame's stream (`stream`); returns at once."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        _abi.check(self._L.ocean_query_velocity_device(self._h, C.byref(s), C.c_void_p(d_xz), int(points), C.c_void_p(d_pos),
                                                       C.c_void_p(d_vel)), "ocean_query_velocity_device")

    def buoyancy_flow(self, bodies, first_tile: int = 0, uv_scales=(1.0,), grid_size: Optional[int] = None,
                      vertex_distance: Optional[float] = None, choppy: float = -1.0, iterations: int = 8, **params):
        """buoyancy() with the drag taken against the moving water (ocean_buoyancy_bodies_flow): the water's velocity under each hull
        point comes from the twins of the cascade set, as in query_velocity.  Same arguments and results as buoyancy()."""
        w = self._body_words(bodies)
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        p = self.buoyancy_params(**params)
        force = np.empty((w.shape[0], 4), dtype=np.float32)
        torque = np.empty_like(force)
        _abi.check(self._L.ocean_buoyancy_bodies_flow(self._h, C.byref(s), C.byref(p), w.ctypes.data_as(C.c_void_p), w.shape[0],
                                                      force.ctypes.data_as(C.c_void_p), torque.ctypes.data_as(C.c_void_p)),
                   "ocean_buoyancy_bodies_flow")
        return force, torque

    def buoyancy_flow_device(self, d_bodies: int, count: int, d_force: int, d_torque: int, first_tile: int = 0, uv_scales=(1.0,),
                             grid_size: Optional[int] = None, vertex_distance: Optional[float] = None, choppy: float = -1.0,
                             iterations: int = 8, **params):
        """buoyancy_flow on device arrays of the context's device (ocean_buoyancy_bodies_flow_device), as buoyancy_device."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        p = self.buoyancy_params(**params)
        _abi.check(self._L.ocean_buoyancy_bodies_flow_device(self._h, C.byref(s), C.byref(p), C.c_void_p(d_bodies), int(count),
                                                             C.c_void_p(d_force), C.c_void_p(d_torque)), "ocean_buoyancy_bodies_flow_device")

    def build_mips(self, tile: int = 0):
        """Mip chain of both maps of `tile` (ocean_build_mips: the reference's s_kUseMipMapping path, Texture2D.cpp:228-330):
        returns (disp_levels, nrm_levels), lists of (N >> l, N >> l, 4) float32 arrays for l = 1 .. log2 N."""
        _abi.check(self._L.ocean_build_mips(self._h, tile), "ocean_build_mips")
        return self._read_chains("ocean_read_mips")

    def _read_chains(self, call: str, *tile):
        """The two packed chains `call` (an ocean_read_* of the C ABI, with its arguments between the context and the two pointers)
        copies out, each split into its levels: two lists of (N >> l, N >> l, 4) float32 arrays for l = 1 .. log2 N."""
        a = np.empty((int(self._L.ocean_mip_texels(self.tile_size)), 4), dtype=np.float32)
        b = np.empty_like(a)
        _abi.check(getattr(self._L, call)(self._h, *tile, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)), call)
        out_a, out_b, off, w = [], [], 0, self.tile_size // 2
        while w >= 1:
            out_a.append(a[off:off + w * w].reshape(w, w, 4)); out_b.append(b[off:off + w * w].reshape(w, w, 4))
            off += w * w; w //= 2
        return out_a, out_b

    # -- LOD sampling (include/ocean_consumers.h: ocean_build_mips_tiles, ocean_sample_surface_lod, ocean_displace_grid_lod) -----
    def build_mips_tiles(self, first_tile: int = 0, count: Optional[int] = None):
        """Mip chains of both maps of the tiles first_tile .. first_tile+count-1 (default: to the end of the batch) behind the most
        recent frame (ocean_build_mips_tiles): the set the LOD calls read.  Enqueued on the frame's stream; returns at once."""
        n = self.tiles - int(first_tile) if count is None else int(count)
        _abi.check(self._L.ocean_build_mips_tiles(self._h, int(first_tile), n), "ocean_build_mips_tiles")

    def read_mips_tile(self, tile: int):
        """One tile's chains of the set (ocean_read_mips_tile; synchronises): (disp_levels, nrm_levels) as build_mips returns them."""
        return self._read_chains("ocean_read_mips_tile", int(tile))

    def device_mips_tiles(self):
        """(d_disp_mips, d_nrm_mips, first_tile, count, levels) of the set (ocean_device_mips_tiles); the pointers are None without one."""
        d, q = C.c_void_p(), C.c_void_p()
        first, count, levels = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _abi.check(self._L.ocean_device_mips_tiles(self._h, C.byref(d), C.byref(q), C.byref(first), C.byref(count), C.byref(levels)),
                   "ocean_device_mips_tiles")
        return d.value, q.value, first.value, count.value, levels.value

    @staticmethod
    def _lod(scale, max_level) -> "_abi.Lod":
        l = _abi.Lod()
        l.scale, l.max_level = float(scale), int(max_level)
        return l

    def sample_surface_lod(self, xzf, first_tile: int = 0, uv_scales=(1.0,), grid_size: Optional[int] = None,
                           vertex_distance: Optional[float] = None, choppy: float = -1.0, scale: float = 1.0, max_level: int = 0):
        """What the cascade vertex stage would write for vertices at the rest points xzf [points, 3] = (x, z, footprint in mesh metres),
        every cascade read at the mip level that fits its footprint (ocean_sample_surface_lod; needs build_mips_tiles behind the
        most recent frame).  Returns (pos, nrm), each (points, 4) float32: pos = (x + dx, height, z + dz, smallest Jacobian slot),
        nrm = (unit normal, coarsest level used)."""
        q = np.ascontiguousarray(xzf, dtype=np.float32).reshape(-1, 3)
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, 0)
        l = self._lod(scale, max_level)
        pos = np.empty((q.shape[0], 4), dtype=np.float32)
        nrm = np.empty_like(pos)
        _abi.check(self._L.ocean_sample_surface_lod(self._h, C.byref(s), C.byref(l), q.ctypes.data_as(C.c_void_p), q.shape[0],
                                                    pos.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p)), "ocean_sample_surface_lod")
        return pos, nrm

    def sample_surface_lod_device(self, d_xzf: int, points: int, d_pos: int, d_nrm: int, first_tile: int = 0, uv_scales=(1.0,),
                                  grid_size: Optional[int] = None, vertex_distance: Optional[float] = None, choppy: float = -1.0,
                                  scale: float = 1.0, max_level: int = 0):
        """sample_surface_lod on device arrays of the context's device (ocean_sample_surface_lod_device): d_xzf [points][3], d_pos /
        d_nrm [points][4] float32, 16-byte aligned.  Enqueued on the frame's stream (`stream`); returns at once."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, 0)
        l = self._lod(scale, max_level)
        _abi.check(self._L.ocean_sample_surface_lod_device(self._h, C.byref(s), C.byref(l), C.c_void_p(d_xzf), int(points), C.c_void_p(d_pos),
                                                           C.c_void_p(d_nrm)), "ocean_sample_surface_lod_device")

    def displace_grid_lod(self, uv_scales, first_tile: int = 0, grid_size: Optional[int] = None,
                          vertex_distance: Optional[float] = None, choppy: float = -1.0, scale: float = 1.0, max_level: int = 0):
        """displace_grid_cascades with every cascade read at the mip level that fits the grid's vertex spacing (ocean_displace_grid_lod;
        needs build_mips_tiles behind the most recent frame): returns (positions, normals) like displace_grid."""
        sc = np.ascontiguousarray(uv_scales, dtype=np.float32)
        g = self.tile_size if grid_size is None else int(grid_size)
        vd = (1000.0 / 512.0) if vertex_distance is None else float(vertex_distance)
        l = self._lod(scale, max_level)
        _abi.check(self._L.ocean_displace_grid_lod(self._h, first_tile, sc.size, g, vd, sc.ctypes.data_as(C.POINTER(C.c_float)), choppy,
                                                   C.byref(l)), "ocean_displace_grid_lod")
        pos = np.empty(((g + 1) * (g + 1), 4), dtype=np.float32)
        nrm = np.empty_like(pos)
        _abi.check(self._L.ocean_read_grid(self._h, pos.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p)), "ocean_read_grid")
        return pos, nrm

    # -- surface bounds (include/ocean_consumers.h: ocean_build_bounds_tiles, ocean_patch_bounds) ---------------------------------
    def build_bounds_tiles(self, first_tile: int = 0, count: Optional[int] = None, first_level: int = 1):
        """Min/max pyramids of the displacement maps of the tiles first_tile .. first_tile+count-1 (default: to the end of the batch)
        behind the most recent frame (ocean_build_bounds_tiles): the set patch_bounds reads.  Levels below first_level are not stored.
        Enqueued on the frame's stream; returns at once."""
        n = self.tiles - int(first_tile) if count is None else int(count)
        _abi.check(self._L.ocean_build_bounds_tiles(self._h, int(first_tile), n, int(first_level)), "ocean_build_bounds_tiles")

    def read_bounds_tile(self, tile: int):
        """One tile's chains of the set (ocean_read_bounds_tile; synchronises): a list of (lo, hi) per level l = 1 .. log2 N, each
        (N >> l, N >> l, 4) float32.  Levels below the set's first_level hold nothing that is specified."""
        return list(zip(*self._read_chains("ocean_read_bounds_tile", int(tile))))

    def device_bounds_tiles(self):
        """(d_lo, d_hi, first_tile, count, levels, first_level) of the set (ocean_device_bounds_tiles); the pointers are None without one."""
        lo, hi = C.c_void_p(), C.c_void_p()
        first, count, levels, first_level = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _abi.check(self._L.ocean_device_bounds_tiles(self._h, C.byref(lo), C.byref(hi), C.byref(first), C.byref(count), C.byref(levels),
                                                     C.byref(first_level)), "ocean_device_bounds_tiles")
        return lo.value, hi.value, first.value, count.value, levels.value, first_level.value

    @staticmethod
    def _patch_query(planes, pad_texels) -> "_abi.PatchQuery":
        q = _abi.PatchQuery()
        pl = np.zeros((0, 4), np.float32) if planes is None else np.asarray(planes, dtype=np.float32).reshape(-1, 4)
        if len(pl) > 6:
            raise ValueError("planes: at most 6")
        q.pad_texels, q.planes = int(pad_texels), len(pl)
        for k, row in enumerate(pl):
            for j in range(4):
                q.plane[k][j] = float(row[j])
        return q

    def patch_bounds(self, rects, first_tile: int = 0, uv_scales=(1.0,), grid_size: Optional[int] = None,
                     vertex_distance: Optional[float] = None, planes=None, pad_texels: int = 0):
        """World-space boxes of the displaced surface over the rest-space rectangles rects [count, 4] = (x0, z0, x1, z1 in mesh metres)
        (ocean_patch_bounds; needs build_bounds_tiles behind the most recent frame).  Returns (lo, hi), each (count, 4) float32:
        lo = (min x, min y, min z, lower bound of the Jacobian slot), hi = (max x, max y, max z, class).  planes [k, 4], k <= 6, rows
        (a, b, c, d) with inside where a*x + b*y + c*z + d >= 0: class 0 outside, 1 straddles, 2 inside; without planes the class is 1."""
        r = np.ascontiguousarray(rects, dtype=np.float32).reshape(-1, 4)
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, 0.0, 0)
        q = self._patch_query(planes, pad_texels)
        lo = np.empty((r.shape[0], 4), dtype=np.float32)
        hi = np.empty_like(lo)
        _abi.check(self._L.ocean_patch_bounds(self._h, C.byref(s), C.byref(q), r.ctypes.data_as(C.c_void_p), r.shape[0],
                                              lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)), "ocean_patch_bounds")
        return lo, hi

    def patch_bounds_device(self, d_rects: int, count: int, d_lo: int, d_hi: int, first_tile: int = 0, uv_scales=(1.0,),
                            grid_size: Optional[int] = None, vertex_distance: Optional[float] = None, planes=None, pad_texels: int = 0):
        """patch_bounds on device arrays of the context's device (ocean_patch_bounds_device): d_rects [count][4], d_lo / d_hi
        [count][4] float32, 16-byte aligned.  Enqueued on the frame's stream (`stream`); returns at once."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, 0.0, 0)
        q = self._patch_query(planes, pad_texels)
        _abi.check(self._L.ocean_patch_bounds_device(self._h, C.byref(s), C.byref(q), C.c_void_p(d_rects), int(count), C.c_void_p(d_lo),
                                                     C.c_void_p(d_hi)), "ocean_patch_bounds_device")

    # -- spray emitters (include/ocean_consumers.h: ocean_emit_spray) ----------------------------------------------------------------
    def _spray(self, s, window, params) -> "_abi.Spray":
        p = _abi.Spray()
        self._L.ocean_default_spray(C.byref(p))
        half = s.grid_size // 2
        p.ix0, p.iy0, p.nx, p.ny = (-half, -half, s.grid_size + 1, s.grid_size + 1) if window is None else (int(x) for x in window)
        for k, v in params.items():
            if k not in ("threshold", "gain", "min_rise", "thin_log2", "salt"):
                raise TypeError(f"emit_spray: unknown parameter {k}")
            setattr(p, k, v)
        return p

    def emit_spray(self, capacity: int, window=None, first_tile: int = 0, uv_scales=(1.0,), grid_size: Optional[int] = None,
                   vertex_distance: Optional[float] = None, out=None, **params):
        """The breaking vertices of a window of the cascade vertex stage's grid on the most recent frame (ocean_emit_spray), in ascending
        lattice index.  window = (ix0, iy0, nx, ny) in grid vertices, default the whole grid (-half, -half, grid_size + 1, grid_size + 1);
        params: threshold, gain, min_rise, thin_log2, salt of ocean_spray.  Returns (pos, vel, index, total): the rows that were written,
        min(total, capacity) of them -- pos (n, 4) = (x, y, z, strength), vel (n, 4) = (V.x, V.y, V.z, J), index (n,) uint32 -- and the
        number of breaking vertices in the window, not capped: capacity = 0 only counts.  out = (pos, vel, index) arrays of `capacity`
        rows (float32, float32, uint32; C-contiguous) are written in place -- rows past the written ones keep what they held -- and the
        results are views of them."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, 0.0, 0)
        p = self._spray(s, window, params)
        capacity = int(capacity)
        if out is None:
            out = (np.empty((capacity, 4), np.float32), np.empty((capacity, 4), np.float32), np.empty(capacity, np.uint32))
        pos, vel, index = out
        for a, dt, shape in ((pos, np.float32, (capacity, 4)), (vel, np.float32, (capacity, 4)), (index, np.uint32, (capacity,))):
            if a.dtype != dt or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError("emit_spray: out = (pos, vel, index) of capacity rows: float32 [capacity, 4] twice, uint32 [capacity]")
        count = (C.c_uint32 * 2)()
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if capacity else None
        _abi.check(self._L.ocean_emit_spray(self._h, C.byref(s), C.byref(p), capacity, ptr(pos), ptr(vel), ptr(index), count), "ocean_emit_spray")
        n = int(count[1])
        return pos[:n], vel[:n], index[:n], int(count[0])

    def emit_spray_device(self, capacity: int, d_pos: int, d_vel: int, d_index: int, d_count: int, window=None, first_tile: int = 0,
                          uv_scales=(1.0,), grid_size: Optional[int] = None, vertex_distance: Optional[float] = None, **params):
        """emit_spray on device arrays of the context's device (ocean_emit_spray_device): d_pos / d_vel [capacity][4] float32 (16-byte
        aligned), d_index [capacity] uint32, d_count [2] uint32 = (total, rows written).  Enqueued on the frame's stream (`stream`);
        returns at once."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, 0.0, 0)
        p = self._spray(s, window, params)
        _abi.check(self._L.ocean_emit_spray_device(self._h, C.byref(s), C.byref(p), int(capacity), C.c_void_p(d_pos), C.c_void_p(d_vel),
                                                   C.c_void_p(d_index), C.c_void_p(d_count)), "ocean_emit_spray_device")

    # -- Gerstner proxy (include/ocean_consumers.h: ocean_extract_waves, ocean_eval_waves, ocean_query_waves) -------------------------
    def extract_waves(self, max_waves: int, tile: int = 0):
        """The tile's strongest spectrum bins as its wave set (ocean_extract_waves): (rows, energy) -- rows a WAVE_DTYPE record array in
        rank order (power descending, ties by bin), count = min(max_waves, bins with power > 0) of them; energy = sum |h0|^2 over the
        rows as float64 (divide by spectrum_moments()[0] for the captured share of the variance).  The set stays on the device for
        eval_waves / query_waves.  Synchronises."""
        rows = np.zeros(max(int(max_waves), 1), dtype=WAVE_DTYPE)
        count, energy = C.c_uint32(0), C.c_double(0.0)
        _abi.check(self._L.ocean_extract_waves(self._h, int(tile), int(max_waves), rows.ctypes.data_as(C.c_void_p), C.byref(count),
                                               C.byref(energy)), "ocean_extract_waves")
        return rows[:count.value], float(energy.value)

    def set_waves(self, rows, tile: int = 0):
        """Upload a hand-made wave set (ocean_set_waves): rows a WAVE_DTYPE record array of at most 4096 rows; none drops the set."""
        rows = np.ascontiguousarray(rows, dtype=WAVE_DTYPE).reshape(-1)
        _abi.check(self._L.ocean_set_waves(self._h, int(tile), rows.ctypes.data_as(C.c_void_p) if len(rows) else None, len(rows)), "ocean_set_waves")

    def get_waves(self, tile: int = 0) -> np.ndarray:
        """The tile's wave set as a WAVE_DTYPE record array (ocean_get_waves).  Synchronises."""
        count = C.c_uint32(0)
        _abi.check(self._L.ocean_get_waves(self._h, int(tile), None, C.byref(count)), "ocean_get_waves")
        rows = np.zeros(count.value, dtype=WAVE_DTYPE)
        _abi.check(self._L.ocean_get_waves(self._h, int(tile), rows.ctypes.data_as(C.c_void_p), C.byref(count)), "ocean_get_waves")
        return rows

    def _waves_call(self, fn, name, xz, t, s):
        q = np.ascontiguousarray(xz, dtype=np.float32).reshape(-1, 2)
        pos = np.empty((q.shape[0], 4), dtype=np.float32)
        nrm = np.empty_like(pos)
        _abi.check(fn(self._h, C.byref(s), float(t), q.ctypes.data_as(C.c_void_p), q.shape[0], pos.ctypes.data_as(C.c_void_p),
                      nrm.ctypes.data_as(C.c_void_p)), name)
        return pos, nrm

    def eval_waves(self, xz, t: float, first_tile: int = 0, uv_scales=(1.0,), grid_size: Optional[int] = None,
                   vertex_distance: Optional[float] = None, choppy: float = -1.0):
        """Forward evaluation of the wave sets of tiles first_tile .. first_tile+len(uv_scales)-1 at rest points xz [points, 2] and time t
        (ocean_eval_waves): no frame is read.  Returns (pos, nrm), each (points, 4) float32: pos = (x, height, z, smallest diagonal
        Jacobian), nrm = (unit normal, 0).  Defaults as displace_grid."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, 0)
        return self._waves_call(self._L.ocean_eval_waves, "ocean_eval_waves", xz, t, s)

    def query_waves(self, xz, t: float, first_tile: int = 0, uv_scales=(1.0,), grid_size: Optional[int] = None,
                    vertex_distance: Optional[float] = None, choppy: float = -1.0, iterations: int = 8):
        """The water of the wave sets above world points xz [points, 2] at time t (ocean_query_waves): query_surface's Newton iteration
        on the analytic evaluation.  Returns (pos, nrm) as query_surface: nrm[:, 3] is the residual |P.xz - xz| in metres."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        return self._waves_call(self._L.ocean_query_waves, "ocean_query_waves", xz, t, s)

    def eval_waves_device(self, d_xz: int, points: int, d_pos: int, d_nrm: int, t: float, first_tile: int = 0, uv_scales=(1.0,),
                          grid_size: Optional[int] = None, vertex_distance: Optional[float] = None, choppy: float = -1.0):
        """eval_waves on device arrays of the context's device (ocean_eval_waves_device): d_xz [points][2], d_pos / d_nrm [points][4]
        float32.  Enqueued on the consumers' stream (`stream`); returns at once."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, 0)
        _abi.check(self._L.ocean_eval_waves_device(self._h, C.byref(s), float(t), C.c_void_p(d_xz), int(points), C.c_void_p(d_pos),
                                                   C.c_void_p(d_nrm)), "ocean_eval_waves_device")

    def query_waves_device(self, d_xz: int, points: int, d_pos: int, d_nrm: int, t: float, first_tile: int = 0, uv_scales=(1.0,),
                           grid_size: Optional[int] = None, vertex_distance: Optional[float] = None, choppy: float = -1.0,
                           iterations: int = 8):
        """query_waves on device arrays (ocean_query_waves_device), as eval_waves_device."""
        s = self._surface(first_tile, uv_scales, grid_size, vertex_distance, choppy, iterations)
        _abi.check(self._L.ocean_query_waves_device(self._h, C.byref(s), float(t), C.c_void_p(d_xz), int(points), C.c_void_p(d_pos),
                                                    C.c_void_p(d_nrm)), "ocean_query_waves_device")

    # -- fragment stage (include/ocean_consumers.h: ocean_sky_radiance, ocean_eval_seabed, ocean_shade_points, ocean_shade_grid) ------------
    def device_grid(self):
        """(d_positions, d_normals, vertices) of the vertex stage's output buffers (ocean_device_grid): what shade_grid shades."""
        d, q, v = C.c_void_p(), C.c_void_p(), C.c_uint32(0)
        _abi.check(self._L.ocean_device_grid(self._h, C.byref(d), C.byref(q), C.byref(v)), "ocean_device_grid")
        return d.value, q.value, v.value

    def sky_radiance(self, dirs, sky=None):
        """SkyPreetham.frag for view directions dirs [count, 3] (ocean_sky_radiance; normalised by the call): (count, 4) float32,
        (r, g, b, sun disk), not tone-mapped.  sky: a struct from sky_params(), or None for the defaults.  Needs no Prepare."""
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        out = np.empty((d.shape[0], 4), dtype=np.float32)
        s = sky_params() if sky is None else sky
        _abi.check(self._L.ocean_sky_radiance(self._h, C.byref(s), d.ctypes.data_as(C.c_void_p), d.shape[0], out.ctypes.data_as(C.c_void_p)),
                   "ocean_sky_radiance")
        return out

    def sky_radiance_device(self, d_dirs, count: int, d_out, sky=None):
        """sky_radiance on device arrays (ocean_sky_radiance_device): torch tensors or pointers, dirs [count][3], out [count][4] float32."""
        s = sky_params() if sky is None else sky
        _abi.check(self._L.ocean_sky_radiance_device(self._h, C.byref(s), _dev_ptr(d_dirs), int(count), _dev_ptr(d_out)), "ocean_sky_radiance_device")

    def eval_seabed(self, xz):
        """The reference's procedural seabed at terrain points xz [count, 2] (ocean_eval_seabed): (count, 4) float32, (unit normal,
        colour factor in [0.6, 0.9]).  Needs no Prepare."""
        q = np.ascontiguousarray(xz, dtype=np.float32).reshape(-1, 2)
        out = np.empty((q.shape[0], 4), dtype=np.float32)
        _abi.check(self._L.ocean_eval_seabed(self._h, q.ctypes.data_as(C.c_void_p), q.shape[0], out.ctypes.data_as(C.c_void_p)), "ocean_eval_seabed")
        return out

    def eval_seabed_device(self, d_xz, count: int, d_out):
        """eval_seabed on device arrays (ocean_eval_seabed_device): torch tensors or pointers, xz [count][2], out [count][4] float32."""
        _abi.check(self._L.ocean_eval_seabed_device(self._h, _dev_ptr(d_xz), int(count), _dev_ptr(d_out)), "ocean_eval_seabed_device")

    def shade_points(self, pos, nrm, sky=None, water=None, aux: bool = False):
        """The reference's water colour for (position, normal) rows [count, 4] as the vertex stage, the queries and the ray cast write
        them (ocean_shade_points): rgba (count, 4) float32, and with aux=True also (p_g.x, p_g.z, t_g, F_r) per point.  sky / water:
        structs from sky_params() / water_params(), or None for the reference's defaults."""
        p = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 4)
        n = np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 4)
        if p.shape != n.shape:
            raise ValueError("pos and nrm: the same number of rows")
        rgba = np.empty_like(p)
        ax = np.empty_like(p) if aux else None
        s = sky_params() if sky is None else sky
        w = water_params() if water is None else water
        _abi.check(self._L.ocean_shade_points(self._h, C.byref(s), C.byref(w), p.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p),
                                              p.shape[0], rgba.ctypes.data_as(C.c_void_p), ax.ctypes.data_as(C.c_void_p) if aux else None),
                   "ocean_shade_points")
        return (rgba, ax) if aux else rgba

    def shade_points_device(self, d_pos, d_nrm, count: int, d_rgba, d_aux=None, sky=None, water=None):
        """shade_points on device arrays (ocean_shade_points_device): torch tensors or pointers, [count][4] float32 each, 16-byte aligned;
        d_aux may be None.  Enqueued on the consumers' stream (`stream`); returns at once."""
        s = sky_params() if sky is None else sky
        w = water_params() if water is None else water
        _abi.check(self._L.ocean_shade_points_device(self._h, C.byref(s), C.byref(w), _dev_ptr(d_pos), _dev_ptr(d_nrm), int(count),
                                                     _dev_ptr(d_rgba), _dev_ptr(d_aux)), "ocean_shade_points_device")

    def shade_grid(self, sky=None, water=None):
        """Shade the vertex stage's output -- the most recent displace_grid, _cascades or _lod -- into the context's image
        (ocean_shade_grid).  Enqueued behind that vertex stage; read_shaded copies the image out."""
        s = sky_params() if sky is None else sky
        w = water_params() if water is None else water
        _abi.check(self._L.ocean_shade_grid(self._h, C.byref(s), C.byref(w)), "ocean_shade_grid")

    def device_shaded(self):
        """(d_rgba, vertices) of the shaded image (ocean_device_shaded); (None, 0) while there is none."""
        d, v = C.c_void_p(), C.c_uint32(0)
        _abi.check(self._L.ocean_device_shaded(self._h, C.byref(d), C.byref(v)), "ocean_device_shaded")
        return d.value, v.value

    def read_shaded(self) -> np.ndarray:
        """The shaded image as (vertices, 4) float32 (ocean_read_shaded).  Synchronises."""
        _, v = self.device_shaded()
        out = np.empty((max(v, 1), 4), dtype=np.float32)
        _abi.check(self._L.ocean_read_shaded(self._h, out.ctypes.data_as(C.c_void_p)), "ocean_read_shaded")
        return out[:v]

    def export_maps(self):
        """dma-buf of the current map set (ocean_export_maps): (fd, disp_offset, nrm_offset, bytes, map_set); close the fd yourself."""
        fd, ms = C.c_int(-1), C.c_int(0)
        do, no, nb = C.c_size_t(), C.c_size_t(), C.c_size_t()
        _abi.check(self._L.ocean_export_maps(self._h, C.byref(fd), C.byref(do), C.byref(no), C.byref(nb), C.byref(ms)), "ocean_export_maps")
        return fd.value, do.value, no.value, nb.value, ms.value

    def bind_output_dmabuf(self, fd: int, nbytes: int, disp_offset: int, nrm_offset: int):
        """Write the maps into memory another owner exported as a dma-buf (ocean_bind_output_dmabuf)."""
        _abi.check(self._L.ocean_bind_output_dmabuf(self._h, fd, nbytes, disp_offset, nrm_offset), "ocean_bind_output_dmabuf")

    def bind_output(self, d_disp: int | None, d_nrm: int | None):
        _abi.check(self._L.ocean_bind_output(self._h, C.c_void_p(d_disp), C.c_void_p(d_nrm)), "ocean_bind_output")

    def set_mode(self, mode: int):
        _abi.check(self._L.ocean_set_mode(self._h, mode), "ocean_set_mode")

    def set_dispersion(self, kind: int, param: float = 0.0):
        """0 deep water (reference), 1 finite depth (param = D), 2 capillary (param = L); next prepare()."""
        _abi.check(self._L.ocean_set_dispersion(self._h, kind, param), "ocean_set_dispersion")

    def set_spectrum_precision(self, bits: int):
        _abi.check(self._L.ocean_set_spectrum_precision(self._h, bits), "ocean_set_spectrum_precision")

    def set_intermediate_precision(self, bits: int):
        """32 (default) or 16: half2 intermediates between the two passes (config 4's reduced mode); next prepare()."""
        _abi.check(self._L.ocean_set_intermediate_precision(self._h, bits), "ocean_set_intermediate_precision")

    def set_pipeline_depth(self, depth: int):
        _abi.check(self._L.ocean_set_pipeline_depth(self._h, depth), "ocean_set_pipeline_depth")

    def set_merged_xpass(self, on: bool):
        _abi.check(self._L.ocean_set_merged_xpass(self._h, int(bool(on))), "ocean_set_merged_xpass")

    def set_start_ramp(self, on: bool):
        _abi.check(self._L.ocean_set_start_ramp(self._h, int(bool(on))), "ocean_set_start_ramp")

    def set_external_readers(self, on: bool):
        _abi.check(self._L.ocean_set_external_readers(self._h, int(bool(on))), "ocean_set_external_readers")

    @property
    def stream(self) -> int:
        return self._L.ocean_stream(self._h) or 0

    def set_stream(self, s: int | None):
        _abi.check(self._L.ocean_set_stream(self._h, C.c_void_p(s)), "ocean_set_stream")

    def select_streams(self, frames: int = 50):
        """Put the context's work on the fastest of the process's hardware queues (ocean_select_streams): times `frames` serial frames on
        each of its first four streams and re-orders them; returns the four frame times in microseconds, fastest first."""
        us = (C.c_float * 4)()
        _abi.check(self._L.ocean_select_streams(self._h, frames, us), "ocean_select_streams")
        return [float(x) for x in us]

    def read_spectrum(self, tile: int = 0):
        n = self.tile_size
        h0 = np.empty((n, n, 2), dtype=np.float32)
        om = np.empty((n, n), dtype=np.float32)
        _abi.check(self._L.ocean_read_spectrum(self._h, tile, h0.ctypes.data_as(C.c_void_p),
                                               om.ctypes.data_as(C.c_void_p)), "ocean_read_spectrum")
        return h0, om

    def read_xi(self, tile: int = 0):
        n = self.tile_size
        xi = np.empty((n, n, 2), dtype=np.float32)
        _abi.check(self._L.ocean_read_xi(self._h, tile, xi.ctypes.data_as(C.c_void_p)), "ocean_read_xi")
        return xi

    def time_frames(self, t0: float, dt: float, warmup: int, frames: int, per_kernel: bool = True):
        """(ms_total, [ms per launch, in kernel_names() order]) measured with HIP events on the launch stream."""
        total = C.c_float()
        k = (C.c_float * 3)()
        _abi.check(self._L.ocean_time_frames(self._h, t0, dt, warmup, frames, C.byref(total),
                                             k if per_kernel else None), "ocean_time_frames")
        return total.value, [k[0], k[1], k[2]] if per_kernel else None

    def kernel_names(self):
        return [self._L.ocean_kernel_name(self._h, i).decode() for i in range(3)]

    def last_launch(self):
        """What the most recent frame launched: three dicts (ocean_launch_info) in kernel_names() order."""
        out = []
        for i in range(3):
            li = _abi.LaunchInfo()
            _abi.check(self._L.ocean_last_launch(self._h, i, C.byref(li)), "ocean_last_launch")
            out.append({k: int(getattr(li, k)) for k, _ in _abi.LaunchInfo._fields_})
        return out

    @property
    def algorithmic_bytes_per_texel(self) -> int:
        return int(self._L.ocean_algorithmic_bytes_per_texel(self._h))

    def algorithmic_bytes_per_launch(self):
        """Bytes per texel of each of the three launches, in kernel_names() order (sums to algorithmic_bytes_per_texel)."""
        return [int(self._L.ocean_algorithmic_bytes_per_launch(self._h, i)) for i in range(3)]


def comm_unique_id() -> bytes:
    """128-byte RCCL id created by one rank and handed to every rank's comm_init."""
    buf = C.create_string_buffer(_abi.OCEAN_COMM_ID_BYTES)
    _abi.check(_abi.lib().ocean_comm_unique_id(buf), "ocean_comm_unique_id")
    return buf.raw


def host_register(arr: np.ndarray):
    _abi.check(_abi.lib().ocean_host_register(arr.ctypes.data_as(C.c_void_p), arr.nbytes), "ocean_host_register")


def host_unregister(arr: np.ndarray):
    _abi.check(_abi.lib().ocean_host_unregister(arr.ctypes.data_as(C.c_void_p)), "ocean_host_unregister")


class WSTessendorf:
    """Drop-in mirror of the reference class (WSTessendorf.h:58-122).

    Like the reference: setters other than SetLambda take effect at the next
    Prepare(); SetTileSize silently ignores a non power of two
    (WSTessendorf.cpp:459-468); nothing raises for "wrong order" except calling
    ComputeWaves before Prepare, which the reference would crash on.
    Prepare() with no seed draws a fresh one, as the reference re-randomises on
    every Prepare (WSTessendorf.cpp:87-103 + core/Application.cpp:21).
    """

    s_kDefaultTileSize = 512
    s_kDefaultTileLength = 1000.0
    s_kDefaultWindDir = (1.0, 1.0)
    s_kDefaultWindSpeed = 30.0
    s_kDefaultAnimPeriod = 200.0
    s_kDefaultPhillipsConst = 3e-7
    s_kDefaultPhillipsDamping = 0.1

    def __init__(self, tileSize: int = 512, tileLength: float = 1000.0, device: int = 0, velocity: bool = False):
        """velocity=True (beyond the reference): the context carries a second tile, the derivative twin of the model's own, which
        QueryVelocity and BuoyancyFlow read (include/WSTessendorf.hpp: withVelocity).  One more tile per frame."""
        if not _is_pow2(tileSize):
            tileSize = self.s_kDefaultTileSize
        self._velocity = bool(velocity)
        self._b = OceanBatch(tileSize, 2 if velocity else 1, device)
        if velocity:
            self._b.set_velocity_twin(1, 0)
        self._b.set_params(tile_length=tileLength)
        self._disp = None
        self._nrm = None
        self._min = -1.0   # WSTessendorf.h:227-228
        self._max = 1.0
        self._seed_ctr = 0
        self._back = None      # pinned back pair of ComputeWavesAsync
        self._pending = None   # (A, min, max) of a ComputeWavesAsync whose copy has not been waited for

    # -- Prepare / ComputeWaves (WSTessendorf.cpp:36-58, 284-455) -------------------
    def Prepare(self, seed: int | None = None, xi: np.ndarray | None = None):
        if seed is None:
            import time
            self._seed_ctr += 1
            seed = (time.time_ns() ^ (self._seed_ctr * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF
        if self._pending is not None:
            self.Wait()
        if self._velocity and xi is not None:       # (the twin's part of injected draws is ignored: the model's own, twice)
            xi = np.stack([np.asarray(xi, dtype=np.float32).reshape(self._b.tile_size, self._b.tile_size, 2)] * 2)
        self._b.prepare(seed, xi)
        n = self._b.tile_size
        self._disp = np.zeros((n, n, 4), dtype=np.float32)            # .cpp:48-51
        self._nrm = np.zeros((n, n, 4), dtype=np.float32)
        self._nrm[..., 1] = 1.0                                        # .cpp:53-54

    def ComputeWaves(self, time: float) -> float:
        if self._pending is not None:
            self.Wait()
        amp = float(self._b.compute_waves(time)[0])
        d, q = self._b.read_maps(0, 1)
        self._disp, self._nrm = d[0], q[0]
        _, self._min, self._max = self._b.heights(0)
        return amp

    # -- opt-in non-blocking pair (include/WSTessendorf.hpp: ComputeWavesAsync / Wait; the reference's DOUBLE_BUFFERED idea,
    #    WaterSurfaceMesh.h:26-34, on the synthesis side) ---------------------------------------------------------------------
    def SelectFastestQueue(self, framesPerQueue: int = 50):
        """Opt-in, once after Prepare(): the model's work on the fastest hardware queue of the process (include/WSTessendorf.hpp)."""
        self.Wait()
        return self._b.select_streams(framesPerQueue)

    def ComputeWavesAsync(self, time: float) -> float:
        """Enqueue the frame and the DMA of both maps into a back pair of pinned arrays; return A as soon as the frame's kernels
        are done (ocean_wait_frame).  GetDisplacements() / GetNormals() keep returning the previous frame until Wait()."""
        if self._pending is not None:
            self.Wait()
        n = self._b.tile_size
        if self._back is None or self._back[0].shape[1] != n:
            self._release_back()
            self._back = (np.zeros((1, n, n, 4), np.float32), np.zeros((1, n, n, 4), np.float32))
            for a in self._back:
                host_register(a)
            self._b.set_frame_tracking(True)
        self._b.compute_waves_async(time)
        self._b.read_maps_async(self._back[0], self._back[1], 0, 1)      # (the model's own tile only: the back pair holds one)
        amp = float(self._b.wait_frame()[0])
        self._pending = self._b.heights(0)
        return amp

    def Wait(self):
        if self._pending is None:
            return
        self._b.synchronize()
        self._disp, self._nrm = self._back[0][0].copy(), self._back[1][0].copy()
        _, self._min, self._max = self._pending
        self._pending = None

    def _release_back(self):
        if getattr(self, "_back", None) is not None:
            for a in self._back:
                try:
                    host_unregister(a)
                except Exception:
                    pass
        self._back = None

    def __del__(self):
        try:
            if self._pending is not None:
                self._b.synchronize()
            self._release_back()
        except Exception:
            pass

    # -- getters (WSTessendorf.h:82-107) ----------------------------------------------
    def GetTileSize(self): return self._b.tile_size
    def GetTileLength(self): return self._b.get_params().tile_length

    def GetWindDir(self):
        p = self._b.get_params()
        inv = 1.0 / math.sqrt(p.wind_dir_x ** 2 + p.wind_dir_y ** 2)
        return (p.wind_dir_x * inv, p.wind_dir_y * inv)

    def GetWindSpeed(self): return max(1e-4, self._b.get_params().wind_speed)
    def GetAnimationPeriod(self): return self._b.get_params().anim_period
    def GetPhillipsConst(self): return self._b.get_params().phillips_const
    def GetDamping(self): return self._b.get_params().damping
    def GetDisplacementLambda(self): return self._b.get_params().lambda_
    def GetMinHeight(self): return self._min
    def GetMaxHeight(self): return self._max
    def GetDisplacementCount(self): return 0 if self._disp is None else self._disp.shape[0] * self._disp.shape[1]
    def GetDisplacements(self): return self._disp
    def GetNormalCount(self): return 0 if self._nrm is None else self._nrm.shape[0] * self._nrm.shape[1]
    def GetNormals(self): return self._nrm

    # -- setters (WSTessendorf.cpp:459-505) ----------------------------------------------
    def SetTileSize(self, size: int):
        if not _is_pow2(size):
            return                      # .cpp:463-467: ignored
        if self._pending is not None:
            self.Wait()
        self._b.set_tile_size(size)

    def SetTileLength(self, length: float): self._b.set_params(tile_length=length)
    def SetWindDirection(self, w): self._b.set_params(wind_dir_x=float(w[0]), wind_dir_y=float(w[1]))
    def SetWindSpeed(self, v: float): self._b.set_params(wind_speed=max(1e-4, v))
    def SetAnimationPeriod(self, T: float): self._b.set_params(anim_period=T)
    def SetPhillipsConst(self, A: float): self._b.set_params(phillips_const=A)
    def SetLambda(self, lam: float): self._b.set_lambda(lam)
    def SetDamping(self, damping: float): self._b.set_params(damping=damping)

    # -- beyond the reference: empirical spectra (include/WSTessendorf.hpp: SetSpectrum / GetSignificantWaveHeight) -------------
    def SetSpectrum(self, **fields):
        """Patch fields of the model's struct ocean_spectrum (kind, spreading, fetch, ... k_min, k_max, scale); next Prepare()."""
        self._b.set_spectrum(0, **fields)

    def GetSignificantWaveHeight(self) -> float:
        """Hs = 4 sqrt(sum |h0|^2) of the prepared spectrum, in metres for an empirical kind (ocean_spectrum_moments)."""
        return 4.0 * math.sqrt(float(self._b.spectrum_moments(0)[0]))

    # -- beyond the reference: surface query (include/WSTessendorf.hpp: QuerySurface) -----------------------------------
    def QuerySurface(self, xz, positions: np.ndarray | None = None, normals: np.ndarray | None = None, iterations: int = 8):
        """Displaced position and normal of the water above each world point xz [points, 2] (ocean_query_surface), for the maps of the
        last ComputeWaves on the reference mesh's geometry: grid = tile size, vertex distance = s_kDefaultTileLength /
        s_kDefaultTileSize (WaterSurfaceMesh.h:200-202), choppy = GetDisplacementLambda().  Fills positions / normals [points, 4]
        float32 when given, and returns them."""
        pos, nrm = self._b.query_surface(xz, grid_size=self._b.tile_size,
                                         vertex_distance=self.s_kDefaultTileLength / self.s_kDefaultTileSize,
                                         choppy=self.GetDisplacementLambda(), iterations=iterations)
        if positions is not None:
            positions[...] = pos.reshape(positions.shape)
            pos = positions
        if normals is not None:
            normals[...] = nrm.reshape(normals.shape)
            nrm = normals
        return pos, nrm

    # -- beyond the reference: ray cast (include/WSTessendorf.hpp: RaycastSurface) ---------------------------------------
    def RaycastSurface(self, origins, directions, max_distance: float, hits: np.ndarray | None = None, normals: np.ndarray | None = None,
                       steps: int = 0, refine: int = 0, iterations: int = 8):
        """Where each ray origins[i] + t * directions[i] ([rays, 3]) first meets the water within max_distance metres
        (ocean_raycast_surface), on the geometry of QuerySurface.  Fills hits / normals [rays, 4] float32 when given, and returns
        them: hits = (x, height, z, t; -2 for an origin under water, -1 for a miss), normals = (unit normal, signed gap or depth)."""
        hit, nrm = self._b.raycast_surface(origins, directions, max_distance, steps, refine, grid_size=self._b.tile_size,
                                           vertex_distance=self.s_kDefaultTileLength / self.s_kDefaultTileSize,
                                           choppy=self.GetDisplacementLambda(), iterations=iterations)
        if hits is not None:
            hits[...] = hit.reshape(hits.shape)
            hit = hits
        if normals is not None:
            normals[...] = nrm.reshape(normals.shape)
            nrm = normals
        return hit, nrm

    # -- beyond the reference: persistent foam (include/WSTessendorf.hpp: UpdateFoam / GetFoam / QueryFoam) -----------------
    def UpdateFoam(self, dt: float, **params):
        """One foam step of dt seconds behind the last ComputeWaves (ocean_update_foam; the library's defaults unless given)."""
        self._b.update_foam(dt, 0, **params)

    def GetFoam(self) -> np.ndarray:
        """Foam coverage (N, N) float32 in [0, 1], texel for texel beside GetDisplacements() / GetNormals()."""
        return self._b.read_foam(0)

    def QueryFoam(self, xz, out: np.ndarray | None = None, iterations: int = 8):
        """Foam above each world point xz [points, 2] (ocean_query_foam) on the geometry of QuerySurface.  Fills out [points, 4] float32
        when given, and returns it: (foam, rest x, rest z, residual in metres)."""
        res = self._b.query_foam(xz, grid_size=self._b.tile_size, vertex_distance=self.s_kDefaultTileLength / self.s_kDefaultTileSize,
                                 choppy=self.GetDisplacementLambda(), iterations=iterations)
        if out is not None:
            out[...] = res.reshape(out.shape)
            res = out
        return res

    # -- beyond the reference: buoyancy (include/WSTessendorf.hpp: SetHull / Buoyancy) ------------------------------------------
    def SetHull(self, points):
        """The hull sample points [count, 4] (local x, y, z, edge of the cubic cell) of Buoyancy() (ocean_set_hull); kept across Prepare()."""
        self._b.set_hull(points)

    def Buoyancy(self, bodies, forces: np.ndarray | None = None, torques: np.ndarray | None = None, iterations: int = 8, **params):
        """Net force and torque on each floating body (BODY_DTYPE records) from the water of the last ComputeWaves
        (ocean_buoyancy_bodies), on the geometry of QuerySurface; params patch density / gravity / drag.  Fills forces / torques
        [bodies, 4] float32 when given, and returns them: (F, submerged volume), (T about the body origin, largest residual)."""
        f, t = self._b.buoyancy(bodies, grid_size=self._b.tile_size, vertex_distance=self.s_kDefaultTileLength / self.s_kDefaultTileSize,
                                choppy=self.GetDisplacementLambda(), iterations=iterations, **params)
        if forces is not None:
            forces[...] = f.reshape(forces.shape)
            f = forces
        if torques is not None:
            torques[...] = t.reshape(torques.shape)
            t = torques
        return f, t

    # -- beyond the reference: water velocity (include/WSTessendorf.hpp: QueryVelocity / BuoyancyFlow), for velocity=True ------------
    def QueryVelocity(self, xz, positions: np.ndarray | None = None, velocities: np.ndarray | None = None, iterations: int = 8):
        """Velocity of the water particle at each world point xz [points, 2] (ocean_query_velocity) on the geometry of QuerySurface.
        Fills positions / velocities [points, 4] float32 when given, and returns them: positions as QuerySurface, velocities =
        (V.x, V.y, V.z in m/s, residual in metres)."""
        pos, vel = self._b.query_velocity(xz, grid_size=self._b.tile_size, vertex_distance=self.s_kDefaultTileLength / self.s_kDefaultTileSize,
                                          choppy=self.GetDisplacementLambda(), iterations=iterations)
        if positions is not None:
            positions[...] = pos.reshape(positions.shape)
            pos = positions
        if velocities is not None:
            velocities[...] = vel.reshape(velocities.shape)
            vel = velocities
        return pos, vel

    def BuoyancyFlow(self, bodies, forces: np.ndarray | None = None, torques: np.ndarray | None = None, iterations: int = 8, **params):
        """Buoyancy() with the drag taken against the moving water (ocean_buoyancy_bodies_flow)."""
        f, t = self._b.buoyancy_flow(bodies, grid_size=self._b.tile_size, vertex_distance=self.s_kDefaultTileLength / self.s_kDefaultTileSize,
                                     choppy=self.GetDisplacementLambda(), iterations=iterations, **params)
        if forces is not None:
            forces[...] = f.reshape(forces.shape)
            f = forces
        if torques is not None:
            torques[...] = t.reshape(torques.shape)
            t = torques
        return f, t
