"""Empirical spectra restated (helper module of the empirical-spectra tests): include/ocean_consumers.h, "empirical wave spectra", step
for step in float64 numpy on the fp32 kx, kz, ux, uz of oracle.numpy_prepare.  Shares no code with the library.

  resolve      alpha, omega_p, gamma of a spectrum (the host's part: PM constants, the JONSWAP fetch relations, caller overrides);
  frequency    S(omega), TMA's depth factor included -- what the energy tests integrate;
  spreading    D = Q(s) ((1 + c) / 2)^s;
  power        P[n, n] = S D (d omega / dk) / k (2 pi / L)^2 on the lattice, 0 at DC, no band, no scale;
  in_band      the fp32 band test;
  restate_h0   the spectrum ocean_prepare must leave in the tile: complex64 [n, n], row-major like read_spectrum.
"""
from __future__ import annotations

import numpy as np
from scipy.special import gammaln

PHILLIPS, PM, JONSWAP, TMA = 0, 1, 2, 3
COS2S, HASSELMANN = 0, 1
G = 9.81
F32 = np.float32
DEFAULT = dict(kind=PHILLIPS, spreading=COS2S, fetch=100e3, gamma=3.3, depth=20.0, spread_s=8.0, swell=0.0, alpha=0.0, peak_omega=0.0,
               k_min=0.0, k_max=0.0, scale=1.0)


def spectrum(**fields) -> dict:
    """DEFAULT patched by fields; every float goes through fp32, as it does through struct ocean_spectrum."""
    s = dict(DEFAULT)
    for k, v in fields.items():
        assert k in s, k
        s[k] = v
    return {k: (int(v) if k in ("kind", "spreading") else float(F32(v))) for k, v in s.items()}


def wind_speed_f32(wind_speed: float) -> float:
    """U: the fp32 wind speed the library prepares with (at least 1e-4)."""
    return float(F32(max(1e-4, wind_speed)))


def resolve(spec: dict, wind_speed: float):
    """(alpha, omega_p, gamma) in double."""
    U, F = wind_speed_f32(wind_speed), spec["fetch"]
    if spec["kind"] == PM:
        alpha, wp, gamma = 0.0081, 0.855 * G / U, 1.0
    else:
        alpha, wp, gamma = 0.076 * (U * U / (F * G)) ** 0.22, 22.0 * (G * G / (U * F)) ** (1.0 / 3.0), spec["gamma"]
    if spec["alpha"] != 0.0:
        alpha = spec["alpha"]
    if spec["peak_omega"] != 0.0:
        wp = spec["peak_omega"]
    return alpha, wp, gamma


def frequency(w, spec: dict, wind_speed: float):
    """S(omega) for omega > 0 (array or scalar)."""
    alpha, wp, gamma = resolve(spec, wind_speed)
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(over="ignore", under="ignore"):
        sigma = np.where(w <= wp, 0.07, 0.09)
        r = np.exp(-(w - wp) ** 2 / (2.0 * sigma * sigma * wp * wp))
        S = alpha * G * G / w ** 5 * np.exp(-1.25 * (wp / w) ** 4) * gamma ** r
        if spec["kind"] == TMA:
            wh = w * np.sqrt(spec["depth"] / G)
            S = S * np.where(wh <= 1.0, 0.5 * wh * wh, np.where(wh < 2.0, 1.0 - 0.5 * (2.0 - wh) ** 2, 1.0))
    return S


def spreading(c, s):
    """D = Q(s) ((1 + c) / 2)^s for the cosine c of the angle to the wind."""
    c, s = np.asarray(c, dtype=np.float64), np.asarray(s, dtype=np.float64)
    ln_q = (2.0 * s - 1.0) * np.log(2.0) - np.log(np.pi) + 2.0 * gammaln(s + 1.0) - gammaln(2.0 * s + 1.0)
    return np.exp(ln_q) * (0.5 * (1.0 + c)) ** s


def exponent(w, spec: dict, wind_speed: float):
    """The spreading exponent s(omega): spread_s or Hasselmann's, plus the swell term."""
    _, wp, _ = resolve(spec, wind_speed)
    w = np.asarray(w, dtype=np.float64)
    if spec["spreading"] == HASSELMANN:
        mu = -2.33 - 1.45 * (wind_speed_f32(wind_speed) * wp / G - 1.17)
        x = w / wp
        s = np.where(x <= 1.05, 6.97 * x ** 4.06, 9.77 * x ** mu)
    else:
        s = np.full_like(w, spec["spread_s"])
    return s + 16.0 * np.tanh(wp / w) * spec["swell"] ** 2


def wind_unit_f32(wind):
    """The fp32 unit wind vector, as oracle.numpy_prepare forms it."""
    wx, wy = F32(wind[0]), F32(wind[1])
    inv = F32(1.0) / np.sqrt(wx * wx + wy * wy, dtype=F32)
    return F32(wx * inv), F32(wy * inv)


def wavenumber_f32(prep: dict) -> np.ndarray:
    """The fp32 |k| of every bin: sqrtf(kx*kx + kz*kz)."""
    kx, kz = prep["kx"], prep["kz"]
    return np.sqrt((kx * kx + kz * kz).astype(F32), dtype=F32)


def dispersion(k, kind: int, param: float):
    """(omega, d omega / dk), continuous, in double."""
    if kind == 1:
        d = float(F32(param))
        th = np.tanh(k * d)
        w = np.sqrt(G * k * th)
        return w, G * (th + k * d * (1.0 - th * th)) / (2.0 * w)
    if kind == 2:
        ll = float(F32(param))
        kl2 = k * k * ll * ll
        w = np.sqrt(G * k * (1.0 + kl2))
        return w, G * (1.0 + 3.0 * kl2) / (2.0 * w)
    return np.sqrt(G * k), 0.5 * np.sqrt(G / k)


def power(prep: dict, spec: dict, length=1000.0, wind=(1.0, 1.0), wind_speed=30.0, dispersion_kind=(0, 0.0)) -> np.ndarray:
    """P of every lattice bin in double: the expected |h0|^2 for scale 1 and no band; 0 where k <= 1e-5f."""
    klen = wavenumber_f32(prep)
    ok = klen > F32(1e-5)
    k = np.where(ok, klen, F32(1.0)).astype(np.float64)
    wx, wy = wind_unit_f32(wind)
    c = np.clip(prep["ux"].astype(np.float64) * np.float64(wx) + prep["uz"].astype(np.float64) * np.float64(wy), -1.0, 1.0)
    w, dwdk = dispersion(k, int(dispersion_kind[0]), dispersion_kind[1])
    with np.errstate(over="ignore", under="ignore"):
        S = frequency(w, spec, wind_speed)
        D = spreading(c, exponent(w, spec, wind_speed))
        dk = 2.0 * np.pi / np.float64(F32(length))
        P = S * D * dwdk / k * (dk * dk)
    return np.where(ok, P, 0.0)


def in_band(prep: dict, spec: dict) -> np.ndarray:
    """k_min <= k and (k_max == 0 or k < k_max), in fp32."""
    klen = wavenumber_f32(prep)
    k_min, k_max = F32(spec["k_min"]), F32(spec["k_max"])
    return (k_min <= klen) & ((k_max == 0) | (klen < k_max))


def restate_h0(prep: dict, xi: np.ndarray, spec: dict, **sea) -> np.ndarray:
    """h0 = ((s xi.x) sp, (s xi.y) sp) in fp32 with sp = (float)(scale sqrt(P)), (0, 0) at DC and outside the band.  complex64 [n, n].
    sea: length, wind, wind_speed, dispersion_kind as for power().  An empirical kind only."""
    assert spec["kind"] != PHILLIPS
    sp = (spec["scale"] * np.sqrt(power(prep, spec, **sea))).astype(F32)
    s = F32(1.0) / np.sqrt(F32(2.0), dtype=F32)
    xi = np.asarray(xi, dtype=F32)
    keep = in_band(prep, spec) & (wavenumber_f32(prep) > F32(1e-5))
    with np.errstate(under="ignore"):
        re = np.where(keep, ((s * xi[..., 0]).astype(F32) * sp).astype(F32), F32(0))
        im = np.where(keep, ((s * xi[..., 1]).astype(F32) * sp).astype(F32), F32(0))
    return (re + 1j * im).astype(np.complex64)


def variance_integral(spec: dict, wind_speed: float) -> float:
    """m0 = the integral of S over omega from 0 to infinity (scipy.integrate.quad, split at the peak)."""
    from scipy.integrate import quad
    _, wp, _ = resolve(spec, wind_speed)
    f = lambda w: float(frequency(w, spec, wind_speed))
    parts = [quad(f, a, b, epsabs=0.0, epsrel=1e-10, limit=200)[0] for a, b in ((0.05 * wp, wp), (wp, 4.0 * wp), (4.0 * wp, 64.0 * wp))]
    return float(sum(parts) + quad(f, 64.0 * wp, np.inf, epsabs=0.0, epsrel=1e-8)[0])


def ulp_distance(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """|got - want| in units of the fp32 spacing at |want| (at least the spacing of the smallest normal number's binade)."""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    spacing = np.maximum(np.spacing(np.abs(want)), np.spacing(F32(np.finfo(F32).tiny))).astype(np.float64)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / spacing
