"""float32 numpy restatement of the water-velocity calls (include/ocean_consumers.h: ocean_set_velocity_twin, ocean_query_velocity,
ocean_buoyancy_bodies_flow; the kernels are k_derive_spectrum in ocean_aux_kernels.h, k_query_velocity in ocean_velocity_kernels.h and
k_buoyancy_bodies<true> in ocean_buoyancy_kernels.h).  TEST INFRASTRUCTURE ONLY.

The twin spectrum is one fp32 multiply per component.  The query is tests/surface_query.py's Newton iteration (restated here only as
far as the rest point, with that module's own _eval) followed by one more sample per cascade from the twins' displacement maps.  The
flow drag is tests/buoyancy.py's point terms with the water's velocity taken off the point's own.
"""
import numpy as np

import buoyancy as B
import surface_query as Q
from oracle.consumer import sample_linear_repeat

F = np.float32


def derive_spectrum(h0, omega):
    """h0' = i w h0 = (-(w * h0.im), w * h0.re) in fp32: h0 complex64 (or [..., 2] float32), omega float32 of the same shape."""
    h0 = np.asarray(h0)
    if np.iscomplexobj(h0):
        re, im = h0.real.astype(np.float32), h0.imag.astype(np.float32)
    else:
        re, im = h0[..., 0].astype(np.float32), h0[..., 1].astype(np.float32)
    w = np.asarray(omega, dtype=np.float32)
    return np.stack([-(w * im), w * re], axis=-1).astype(np.float32)


def as_complex(h0_pairs):
    return (h0_pairs[..., 0] + 1j * h0_pairs[..., 1]).astype(np.complex64)


def rest_points(disps, nrms, amps, lambdas, lengths, uv_scales, grid, vertex_distance, xz, iterations=8):
    """The K Newton steps of ocean_query_surface from r_0 = q (surface_query.query_surface's loop): (rx, rz) float32."""
    disps = [np.ascontiguousarray(d, dtype=np.float32) for d in disps]
    nrms = [np.ascontiguousarray(q, dtype=np.float32) for q in nrms]
    g = Q.gains(lambdas, lengths, uv_scales, grid, vertex_distance)
    xz = np.ascontiguousarray(xz, dtype=np.float32).reshape(-1, 2)
    qx, qz = xz[:, 0].copy(), xz[:, 1].copy()
    rx, rz = qx.copy(), qz.copy()
    for _ in range(8 if iterations == 0 else int(iterations)):
        dx, _, dz, _, _, _, _, _, jx, jz = Q._eval(disps, nrms, amps, uv_scales, g, grid, vertex_distance, rx, rz)
        ex = (rx + dx) - qx
        ez = (rz + dz) - qz
        rx = rx - ex / Q._clamp(F(1.0) + jx)
        rz = rz - ez / Q._clamp(F(1.0) + jz)
    return rx, rz


def velocity_at(twin_disps, twin_amps, uv_scales, grid, vertex_distance, rx, rz):
    """V at rest points (rx, rz): the twins' displacement maps at the query's uv, summed in cascade order from 0.0f.  [points, 3]."""
    half = F(grid // 2)
    u = (rx / F(vertex_distance) + half) / F(grid)
    v = (rz / F(vertex_distance) + half) / F(grid)
    vx, vy, vz = np.zeros_like(rx), np.zeros_like(rx), np.zeros_like(rx)
    for d, amp, sc in zip(twin_disps, twin_amps, uv_scales):
        sd = sample_linear_repeat(np.ascontiguousarray(d, dtype=np.float32), u * F(sc), v * F(sc))
        vx = vx + sd[:, 0]; vy = vy + sd[:, 1] * F(amp); vz = vz + sd[:, 2]
    return np.stack([vx, vy, vz], axis=1).astype(np.float32)


def query_velocity(disps, nrms, amps, twin_disps, twin_amps, lambdas, lengths, uv_scales, grid, vertex_distance, choppy, xz, iterations=8):
    """(pos, vel), each [points, 4] float32, as ocean_query_velocity: pos is query_surface's, vel = (V, its residual)."""
    pos, nrm = Q.query_surface(disps, nrms, amps, lambdas, lengths, uv_scales, grid, vertex_distance, choppy, xz, iterations)
    rx, rz = rest_points(disps, nrms, amps, lambdas, lengths, uv_scales, grid, vertex_distance, xz, iterations)
    vel = velocity_at(twin_disps, twin_amps, uv_scales, grid, vertex_distance, rx, rz)
    return pos, np.concatenate([vel, nrm[:, 3:]], axis=1).astype(np.float32)


def point_terms_flow(bodies, bi, a, p, e, height, res, water, weight, drag):
    """buoyancy.point_terms with u = (vel + cross(omega, a)) - V, V = water [pairs, 3]: [pairs, 8] float32."""
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.fmin(np.fmax((height - p[1]) / e + F(0.5), F(0.0)), F(1.0))
        v = s * ((e * e) * e)
        om = tuple(bodies["omega"][bi, c] for c in range(3))
        oa = B.cross(om, a)
        u = tuple((bodies["vel"][bi, c] + oa[c]) - water[:, c] for c in range(3))
        dv = F(drag) * v
        f = ((-dv) * u[0], F(weight) * v - dv * u[1], (-dv) * u[2])
        tq = B.cross(a, f)
    return np.stack([f[0], f[1], f[2], tq[0], tq[1], tq[2], v, res], axis=1).astype(np.float32)


def finish_flow(bodies, hull, bi, pi, hi, height, res, water, density, gravity, drag):
    """buoyancy.finish for the flow form: (force, torque, sum of |term| per channel) from the water (height, residual, V) under every pair."""
    a, p, e = B.world_points(hull, bodies, bi, hi)
    terms = point_terms_flow(bodies, bi, a, p, e, height, res, water, F(density) * F(gravity), drag)
    out = B.reduce_bodies(terms, bi, pi, len(bodies))
    mag = np.zeros((len(bodies), 8), np.float64)
    np.add.at(mag, bi, np.abs(terms.astype(np.float64)))
    return out[:, [0, 1, 2, 6]].copy(), out[:, [3, 4, 5, 7]].copy(), mag
