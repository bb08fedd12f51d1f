"""Spectra that make every bin visible, and a reference that needs no FFT (helper module of the spectral-coverage tests).

A Phillips sea -- the input of every other parity test -- falls off as k^-4 exp(-k^2 l^2) and vanishes across the wind, so its
weakest lines are exactly the ones where the z pass has its special cases: index 0 of each axis is the Nyquist frequency
(k = 2 pi (i - N/2) / L), row N/2 is self-mirrored, and the x passes compute columns 0 .. N/2 only and mirror the rest.  A kernel that
dropped the Nyquist column at 4096^2 would still meet the suite's 1e-5.  The inputs here go through the public path,
OceanBatch.prepare(seed, xi): the device computes h0 = (xi / sqrt 2) sqrt P(k), so choosing xi chooses the spectrum.

  white_xi   a flat spectrum: |h0| = AMP on every bin but DC (unit modulus, random phase), so every bin is equally visible;
  edge_xi    the same amplitude on the edge lines only (rows and columns 0, 1, N/2 -+ 1, N/2, N - 1 and the lines either side of
             the z pass's row-block and last-stage boundaries next to N/2); zero elsewhere;
  sparse_xi  about thirty fixed bins with distinct amplitudes and phases -- the four corners, the Nyquist lines' neighbours, the
             self-mirrored row and column, mirror pairs -- and the DC bin, which must contribute nothing;
  closed_form  the float64 maps of a sparse spectrum as a sum of outer products: no FFT at all, so it arbitrates between the
             kernels and the oracle's transforms.

PARAMS: damping 0 (nothing fades at large k) and a wind direction of irrational slope (no lattice bin lies exactly across the
wind, where P = 0); the other parameters are the reference's defaults.
"""
from __future__ import annotations

import functools

import numpy as np

PARAMS = dict(length=1000.0, wind=(1.0, 0.4142135), wind_speed=30.0, anim_period=200.0, phillips_a=3e-7, damping=0.0, lam=-1.0)
AMP = 1e-2              # |h0| of an excited bin
CAP = 1e-6              # bins whose sqrt(P) / sqrt(2) is below AMP * CAP stay unexcited (h0 would leave the normal range of fp32)
MODES = ("full7", "choppy5", "height1", "jacobian")        # = oracle MODE_* = OCEAN_MODE_* 0..3
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)


def gpu_params(params=PARAMS) -> dict:
    """PARAMS as OceanBatch.set_params fields."""
    return dict(tile_length=params["length"], wind_dir_x=params["wind"][0], wind_dir_y=params["wind"][1], wind_speed=params["wind_speed"],
                anim_period=params["anim_period"], phillips_const=params["phillips_a"], damping=params["damping"], lambda_=params["lam"])


def make_oracle(n: int, xi: np.ndarray, params=PARAMS):
    """The C oracle prepared on PARAMS and xi (n, n, 2)."""
    from oracle import oracle as O
    o = O.Oracle(n, **params)
    o.prepare(xi=xi)
    return o


@functools.lru_cache(maxsize=4)
def unit(n: int) -> np.ndarray:
    """Re h0 for xi = 1 on every bin: sqrt(P(k)) / sqrt(2) in the oracle's own fp32 arithmetic (0 at DC)."""
    o = make_oracle(n, np.ones((n, n, 2), np.float32))
    u = o.h0[..., 0].astype(np.float64)
    u.setflags(write=False)
    return u


def _flat(n: int, amp: np.ndarray, rng: np.random.Generator, tiles: int) -> np.ndarray:
    """xi such that h0 = amp * exp(i phi), phi uniform, on every bin with unit >= AMP * CAP; 0 elsewhere.  (tiles, n, n, 2) float32."""
    u = unit(n)
    ok = u >= AMP * CAP
    phi = rng.uniform(0.0, 2.0 * np.pi, size=(tiles, n, n))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(ok, amp / u, 0.0)
    return np.stack([s * np.cos(phi), s * np.sin(phi)], axis=-1).astype(np.float32)


def white_xi(n: int, seed: int, tiles: int = 1) -> np.ndarray:
    """A flat spectrum, |h0| = AMP on every bin but DC and the capped ones; every tile its own phases.  (tiles, n, n, 2)."""
    return _flat(n, np.full((n, n), AMP), np.random.default_rng(seed), tiles)


def edge_lines(n: int) -> list:
    """The lines of edge_xi: 0, 1, N/2 - 1, N/2, N/2 + 1, N - 1, and either side of the z pass's blocks next to N/2 -- row blocks of
    ZB = 8 (16 in the half2 form) in the intermediates (Half<N>::zidx) and the last stage's stride N / 4 or N / 2 (ZStore::pos)."""
    h = n // 2
    lines = {0, 1, h - 1, h, h + 1, n - 1}
    for b in (8, 16, n // 4):
        if b < h:
            lines |= {h - b - 1, h - b, h + b - 1, h + b}
    return sorted(x for x in lines if 0 <= x < n)


def edge_mask(n: int) -> np.ndarray:
    m = np.zeros((n, n), bool)
    lines = edge_lines(n)
    m[lines, :] = True
    m[:, lines] = True
    return m


def edge_xi(n: int, seed: int, tiles: int = 1) -> np.ndarray:
    """white_xi on the edge lines (rows and columns of edge_lines), zero on every other bin.  (tiles, n, n, 2)."""
    return white_xi(n, seed, tiles) * edge_mask(n)[None, :, :, None]


def sparse_bins(n: int) -> list:
    """(row m, column q) of the bins sparse_xi excites; (N/2, N/2) is DC (k = 0)."""
    h, e = n // 2, n - 1
    b = [(0, 0), (0, e), (e, 0), (e, e), (0, 1), (1, 0), (0, h), (h, 0), (1, e), (e, 1),
         (h - 1, h), (h + 1, h), (h, h - 1), (h, h + 1), (h - 1, h + 1), (h + 1, h - 1),
         (1, 1), (h, e), (e, h), (h + 1, 0), (0, h - 1), (3, n - 3), (n - 3, 3), (h - 2, 5 % n), (n // 4, 3 * n // 4),
         (3 * n // 4, n // 4), (h + 3, h - 5), (e - 1, 2), (2, h + 2), (h, h)]
    out = []
    for x in b:
        if x not in out:
            out.append(x)
    return out


def sparse_xi(n: int) -> np.ndarray:
    """The bins of sparse_bins with distinct amplitudes (0.3 .. 1.0 times AMP) and phases; the DC bin gets a xi as well, which the
    spectrum's k = 0 rule must turn into h0 = 0.  (1, n, n, 2)."""
    bins = sparse_bins(n)
    u = unit(n)
    xi = np.zeros((1, n, n, 2), np.float32)
    for j, (m, q) in enumerate(bins):
        if (m, q) == (n // 2, n // 2):
            xi[0, m, q] = (5.0, -3.0)
            continue
        a = AMP * (0.3 + 0.7 * ((j * 7) % len(bins)) / len(bins))
        phi = 2.0 * np.pi * ((j * 0.618034) % 1.0)
        xi[0, m, q] = (a / u[m, q] * np.cos(phi), a / u[m, q] * np.sin(phi))
    return xi


# --------------------------------------------------------------------------------------------------------------------------------
# closed form

def spectrum_of(o) -> dict:
    """What closed_form needs from a prepared oracle: its own k, k-hat, h0 and omega (fp32), copied."""
    return dict(k=o.kvec.copy(), u=o.kunit.copy(), h0=o.h0.copy(), omega=o.omega.copy(), n=o.n)


def coefficients(sp: dict, idx, t: float, jacobian: bool) -> list:
    """[c_f * r] of the bins idx (a tuple of row and column index arrays), f = h, Dx, Dz, slope x, slope z, dxDx, dzDz[, dzDx, dxDz]:
    r = 2 (Re h0 cos wt - Im h0 sin wt) with the fp32 product w t (as numpy_compute_waves), c_f in {1, -i ux, -i uz, i kx, i kz,
    kx ux, kz uz, kz ux, kx uz}."""
    f32 = np.float32
    h0 = sp["h0"][idx]
    wt = (sp["omega"][idx] * f32(t)).astype(f32)
    c, s = np.cos(wt.astype(np.float64)), np.sin(wt.astype(np.float64))
    r = 2.0 * (h0[..., 0].astype(np.float64) * c - h0[..., 1].astype(np.float64) * s)
    kx, kz = (sp["k"][idx][..., i].astype(np.float64) for i in (0, 1))
    ux, uz = (sp["u"][idx][..., i].astype(np.float64) for i in (0, 1))
    cf = [1.0 + 0j, -1j * ux, -1j * uz, 1j * kx, 1j * kz, kx * ux + 0j, kz * uz + 0j]
    if jacobian:
        cf += [kz * ux + 0j, kx * uz + 0j]
    return [c_ * r for c_ in cf]


def _phases(n: int, k: np.ndarray) -> np.ndarray:
    """exp(2 pi i p k / N) for p = 0 .. N-1 (rows) and each k (columns), with the exponent reduced exactly in integers."""
    p = np.arange(n, dtype=np.int64)[:, None]
    return np.exp(2j * np.pi * ((p * np.asarray(k, np.int64)[None, :]) % n) / n)


def pack(fields: list, lam: float, mode: int, n: int):
    """(A, disp, nrm, hmin, hmax) from the signed float64 fields, packed as numpy_compute_waves / the oracle's stages E-G do."""
    h = fields[0]
    hmin = min(float(h.min()), FLT_MAX)
    hmax = max(float(h.max()), FLT_MIN)                                      # max starts at FLT_MIN (reference quirk)
    amp = max(abs(hmin), abs(hmax))
    z = np.zeros_like(h)
    if mode == 2:                                                            # HEIGHT1
        disp = np.stack([z, h / amp, z, z + 1.0], axis=-1)
        return amp, disp, np.zeros((n, n, 4)), hmin, hmax
    dx, dz, sx, sz = fields[1:5]
    if mode == 1:                                                            # CHOPPY5
        return amp, np.stack([lam * dx, h / amp, lam * dz, z + 1.0], axis=-1), np.stack([sx, sz, z, z], axis=-1), hmin, hmax
    dxdx, dzdz = fields[5:7]
    w = z + 1.0
    if mode == 3:                                                            # JACOBIAN
        dzdx, dxdz = fields[7:9]
        w = (1.0 + lam * dxdx) * (1.0 + lam * dzdz) - (lam * dxdz) * (lam * dzdx)
    return amp, np.stack([lam * dx, h / amp, lam * dz, w], axis=-1), np.stack([sx, sz, dxdx, dzdz], axis=-1), hmin, hmax


def closed_form(sp: dict, t: float, lam: float, mode: int):
    """Float64 maps of a sparse spectrum without an FFT: field_f[p, q] = (-1)^(p+q) sum_b Re(c_f(b) r_b exp(2 pi i (p m_b + q n_b) / N))
    over the bins b = (m_b, n_b) with h0 != 0, as two real matrix products per field.  sp: spectrum_of(oracle).  Returns
    (A, disp[N, N, 4], nrm[N, N, 4], hmin, hmax) like numpy_compute_waves."""
    n = sp["n"]
    idx = np.nonzero((sp["h0"] != 0).any(axis=-1))
    sign = 1.0 - 2.0 * ((np.arange(n)[:, None] + np.arange(n)[None, :]) & 1)
    U, V = _phases(n, idx[0]), _phases(n, idx[1]).T                         # U[p, b], V[b, q]
    fields = []
    for cr in coefficients(sp, idx, t, mode == 3)[:{0: 7, 1: 5, 2: 1, 3: 9}[mode]]:
        Uc = U * cr[None, :]
        fields.append(sign * (Uc.real @ V.real - Uc.imag @ V.imag))
    return pack(fields, lam, mode, n)


def impulse_maps(sp: dict, rows: np.ndarray, cols: np.ndarray, t: float, lam: float, mode: int):
    """closed_form of each single bin (rows[i], cols[i]) on its own, vectorised over the bins: (A[B], disp[B, N, N, 4], nrm[B, N, N, 4])."""
    n = sp["n"]
    sign = 1.0 - 2.0 * ((np.arange(n)[:, None] + np.arange(n)[None, :]) & 1)
    U, V = _phases(n, rows).T, _phases(n, cols).T                            # [b, p], [b, q]
    fields = []
    for cr in coefficients(sp, (rows, cols), t, mode == 3)[:{0: 7, 1: 5, 3: 9}[mode]]:
        Uc = U * cr[:, None]
        fields.append(sign[None] * (Uc.real[:, :, None] * V.real[:, None, :] - Uc.imag[:, :, None] * V.imag[:, None, :]))
    h = fields[0]
    hmin = np.minimum(h.min(axis=(1, 2)), FLT_MAX)
    hmax = np.maximum(h.max(axis=(1, 2)), FLT_MIN)
    amp = np.maximum(np.abs(hmin), np.abs(hmax))
    dx, dz, sx, sz, dxdx, dzdz = fields[1:7]
    w = np.ones_like(h)
    if mode == 3:
        dzdx, dxdz = fields[7:9]
        w = (1.0 + lam * dxdx) * (1.0 + lam * dzdz) - (lam * dxdz) * (lam * dzdx)
    disp = np.stack([lam * dx, h / amp[:, None, None], lam * dz, w], axis=-1)
    return amp, disp, np.stack([sx, sz, dxdx, dzdz], axis=-1), hmin, hmax


# --------------------------------------------------------------------------------------------------------------------------------
# error measures

def chan_err(a: np.ndarray, b: np.ndarray) -> list:
    """max|a - b| / max|b| per channel of the last axis (as tests/test_variants_gpu.chan_err)."""
    out = []
    for c in range(a.shape[-1]):
        den = max(float(np.abs(b[..., c]).max()), 1e-30)
        out.append(float(np.abs(a[..., c].astype(np.float64) - b[..., c]).max()) / den)
    return out


def worst_bins(got: np.ndarray, ref: np.ndarray, count: int = 4) -> list:
    """Failure diagnostic: the spectrum bins (row, column) that carry most of a map's error -- the float64 forward FFT of the signed
    residual per channel -- as (channel, (m, q), share of the channel's residual energy)."""
    n = ref.shape[0]
    sign = 1.0 - 2.0 * ((np.arange(n)[:, None] + np.arange(n)[None, :]) & 1)
    out = []
    for c in range(ref.shape[-1]):
        r = np.fft.fft2(sign * (got[..., c].astype(np.float64) - ref[..., c])) / (n * n)
        e = np.abs(r) ** 2
        tot = float(e.sum())
        if tot == 0.0:
            continue
        for j in np.argsort(e, axis=None)[::-1][:count]:
            out.append((c, divmod(int(j), n), round(float(e.flat[j]) / tot, 4)))
    return out
