"""The Gerstner proxy restated in numpy (helper module of tests/test_waves.py and tests/test_waves_gpu.py): the rows of a wave set from
a spectrum (include/ocean_consumers.h: ocean_wave, ocean_extract_waves), their float64 evaluation and Newton inverse (ocean_eval_waves,
ocean_query_waves), and the DERIVED error bound the device is held to.

What is restated bit for bit and what is not
  rows        every field: integer lattice indices, the fp32 wavenumbers, ux = kx * (1 / sqrt(kx*kx + kz*kz)) in fp32, h0, omega, bin.
  selection   the device's own rule -- the 64-bit key (bits of the fp32 power) << 32 | ~bin, the K largest keys in descending order --
              which tests/test_waves.py compares with a plain np.lexsort (power descending, bin ascending).
  position    u, v, the texel coordinate and the fraction of a tile length (fX, fZ) in fp32, operation for operation.
  c_j(t)      the frames' coefficient as numpy_compute_waves forms it: wt one fp32 multiply, cos / sin correctly rounded to fp32, the
              two products, the difference and the doubling in fp32.  This is the reference's own rounding, the "exact" c_j of the bound.
  the sums    float64, phase theta = 2 pi (jx fX + jz fZ) from the fp32 fX, fZ.  Not bit-restatable on the device (sine, cosine, order of
              the sum): held to bound() below.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
WAVES_MAX = 4096
WAVE_DTYPE = np.dtype([("jx", np.int32), ("jz", np.int32), ("kx", f32), ("kz", f32), ("ux", f32), ("uz", f32),
                       ("re", f32), ("im", f32), ("omega", f32), ("bin", np.uint32), ("reserved", f32, 2)])
CHANNELS = ("h", "dx", "dz", "sx", "sz", "xx", "zz")
FLT_MAX = float(np.finfo(f32).max)


# ------------------------------------------------------------------------------------------------------------------------------------
# rows

def k1d(n: int, length: float) -> np.ndarray:
    """The tile's fp32 wavenumbers: float(pi * (2 i - N) / L), the product and quotient in double (oracle.numpy_prepare's k1)."""
    idx = np.arange(n, dtype=np.int32)
    return (np.pi * (f32(2.0) * idx.astype(f32) - f32(n)).astype(np.float64) / np.float64(f32(length))).astype(f32)


def power(h0: np.ndarray) -> np.ndarray:
    """re*re + im*im in fp32, three rounded operations."""
    re, im = h0[..., 0].astype(f32), h0[..., 1].astype(f32)
    return ((re * re).astype(f32) + (im * im).astype(f32)).astype(f32)


def select_bins(h0: np.ndarray, max_waves: int) -> np.ndarray:
    """The bins of the set in rank order by the device's rule: keys (power bits << 32) | ~bin of the candidates (power > 0: never a NaN),
    the largest min(max_waves, candidates) of them, descending."""
    p = power(h0).reshape(-1)
    bins = np.nonzero(p > 0)[0].astype(np.uint64)
    keys = (p[bins.astype(np.int64)].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xffffffff) - bins)
    keys = np.sort(keys)[::-1][:max_waves]
    return (np.uint64(0xffffffff) - (keys & np.uint64(0xffffffff))).astype(np.uint32)


def select_bins_lexsort(h0: np.ndarray, max_waves: int) -> np.ndarray:
    """The same list from the rule as the header words it: power descending, ties by bin ascending."""
    p = power(h0).reshape(-1).astype(np.float64)
    bins = np.nonzero(p > 0)[0]
    order = np.lexsort((bins, -p[bins]))
    return bins[order][:max_waves].astype(np.uint32)


def make_rows(h0: np.ndarray, omega: np.ndarray, k1: np.ndarray, bins: np.ndarray) -> np.ndarray:
    """ocean_wave rows of the given bins (p * N + q) of a spectrum in ocean_read_spectrum's layout: h0 (N, N, 2), omega (N, N)."""
    n = h0.shape[0]
    bins = np.asarray(bins, dtype=np.int64)
    p, q = bins // n, bins % n
    r = np.zeros(len(bins), dtype=WAVE_DTYPE)
    r["jx"], r["jz"] = q - n // 2, p - n // 2
    kx, kz = k1[q].astype(f32), k1[p].astype(f32)
    r["kx"], r["kz"] = kx, kz
    ln = np.sqrt(((kx * kx).astype(f32) + (kz * kz).astype(f32)).astype(f32), dtype=f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (f32(1.0) / ln).astype(f32)
        r["ux"] = np.where(ln <= f32(1e-5), f32(0), (kx * inv).astype(f32))
        r["uz"] = np.where(ln <= f32(1e-5), f32(0), (kz * inv).astype(f32))
    r["re"], r["im"] = h0[p, q, 0], h0[p, q, 1]
    r["omega"] = omega[p, q]
    r["bin"] = bins
    return r


def extract(h0: np.ndarray, omega: np.ndarray, length: float, max_waves: int):
    """(rows, energy) of ocean_extract_waves: energy summed in list order in double."""
    rows = make_rows(h0, omega, k1d(h0.shape[0], length), select_bins(h0, max_waves))
    energy = 0.0
    for re, im in zip(rows["re"].astype(np.float64), rows["im"].astype(np.float64)):
        energy += re * re + im * im
    return rows, energy


def hand_row(n: int, length: float, jx: int, jz: int, re: float, im: float, omega: float) -> np.ndarray:
    """One hand-made row on the tile's lattice."""
    h0 = np.zeros((n, n, 2), f32)
    om = np.zeros((n, n), f32)
    p, q = jz + n // 2, jx + n // 2
    h0[p, q] = (re, im)
    om[p, q] = omega
    return make_rows(h0, om, k1d(n, length), np.array([p * n + q]))


# ------------------------------------------------------------------------------------------------------------------------------------
# evaluation

def coefficients(rows: np.ndarray, tt, double_wt: bool = False) -> np.ndarray:
    """c_j(tt) = 2 (re cos wt - im sin wt) as the frames round it (oracle.numpy_compute_waves), returned as float64."""
    wt = (rows["omega"] * f32(tt)).astype(f32)
    if double_wt:
        wt = (wt * f32(2.0)).astype(f32)
    c, s = np.cos(wt.astype(np.float64)).astype(f32), np.sin(wt.astype(np.float64)).astype(f32)
    return (f32(2.0) * ((rows["re"] * c).astype(f32) - (rows["im"] * s).astype(f32)).astype(f32)).astype(np.float64)


def tile_fraction(x: np.ndarray, n: int, grid: int, vd: float, scale: float) -> np.ndarray:
    """fX of rest coordinate x (fp32 array) for a cascade of uv scale `scale`, in fp32 operation for operation:
    u = (x / vd + half) / grid;  tx = (u * scale) * N - 0.5;  X = tx * (1 / N);  fX = X - floor(X)."""
    x = np.asarray(x, dtype=f32)
    u = ((x / f32(vd)).astype(f32) + f32(grid // 2)).astype(f32) / f32(grid)
    tx = (((u.astype(f32) * f32(scale)).astype(f32) * f32(n)).astype(f32) - f32(0.5)).astype(f32)
    X = (tx * (f32(1.0) / f32(n))).astype(f32)
    return (X - np.floor(X)).astype(f32)


def tile_fraction64(x: np.ndarray, n: int, grid: int, vd: float, scale: float) -> np.ndarray:
    """The same position in float64, not reduced: for the float64 Newton restatement, whose rest points are no fp32 numbers."""
    u = (np.asarray(x, np.float64) / float(f32(vd)) + float(grid // 2)) / float(grid)
    return u * float(f32(scale)) - 0.5 / n


def sums(rows: np.ndarray, c: np.ndarray, X: np.ndarray, Z: np.ndarray, neg_sin: bool = False, shift: int = 0) -> np.ndarray:
    """The seven sums (CHANNELS) of one wave set with coefficients c at positions (X, Z) in tile lengths: float64 [7, points].
    neg_sin / shift (added to jx) are the deliberate mistakes test_waves.py shows the bound catches."""
    jx, jz = rows["jx"].astype(np.float64) + shift, rows["jz"].astype(np.float64)
    kx, kz, ux, uz = (rows[k].astype(np.float64) for k in ("kx", "kz", "ux", "uz"))
    X, Z = np.asarray(X, np.float64).reshape(-1), np.asarray(Z, np.float64).reshape(-1)
    out = np.zeros((7, X.size))
    step = max(1, (1 << 22) // max(len(rows), 1))
    for i in range(0, X.size, step):
        ph = np.outer(X[i:i + step], jx) + np.outer(Z[i:i + step], jz)
        th = 2.0 * np.pi * (ph - np.floor(ph))
        co, si = np.cos(th), np.sin(th) * (-1.0 if neg_sin else 1.0)
        out[0, i:i + step] = co @ c
        out[1, i:i + step] = si @ (ux * c)
        out[2, i:i + step] = si @ (uz * c)
        out[3, i:i + step] = -(si @ (kx * c))
        out[4, i:i + step] = -(si @ (kz * c))
        out[5, i:i + step] = co @ (kx * ux * c)
        out[6, i:i + step] = co @ (kz * uz * c)
    return out


class Surface:
    """The arguments of an evaluation: the wave set, lambda, time offset and tile length of every cascade, the mesh and choppy."""

    def __init__(self, sets, n, lams, lengths, scales, grid, vd, choppy=-1.0, toffs=None):
        self.sets, self.n, self.grid, self.vd, self.choppy = list(sets), int(n), int(grid), float(f32(vd)), float(f32(choppy))
        self.lams = [float(f32(x)) for x in lams]
        self.lengths = [float(f32(x)) for x in lengths]
        self.scales = [float(f32(x)) for x in scales]
        self.toffs = [0.0] * len(self.sets) if toffs is None else [float(f32(x)) for x in toffs]

    def gains(self):
        """lam_c * (s_c * L_c / (grid * vd)) in fp32, as the host forms the Newton step's unit factor."""
        return [float(f32(l) * ((f32(s) * f32(L)).astype(f32) / (f32(self.grid) * f32(self.vd)).astype(f32)).astype(f32))
                for l, s, L in zip(self.lams, self.scales, self.lengths)]


def combine(S: Surface, per, x, z):
    """out_pos, out_nrm (float64 [points, 4]) and the Newton diagonal from the per-cascade sums `per` (list of [7, points])."""
    x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
    px, py, pz = x.copy(), np.zeros_like(x), z.copy()
    s4 = np.zeros((4, x.size))
    J = np.full(x.size, FLT_MAX)
    jx, jz = np.ones_like(x), np.ones_like(x)
    for c, f in enumerate(per):
        lam = S.lams[c]
        px += lam * f[1]; py += f[0]; pz += lam * f[2]
        s4 += f[3:7]
        J = np.minimum(J, (1.0 + lam * f[5]) * (1.0 + lam * f[6]))
        jx += S.gains()[c] * f[5]; jz += S.gains()[c] * f[6]
    nx = -(s4[0] / (1.0 + S.choppy * s4[2]))
    nz = -(s4[1] / (1.0 + S.choppy * s4[3]))
    ln = np.sqrt(nx * nx + 1.0 + nz * nz)
    pos = np.stack([px, py, pz, J], axis=-1)
    nrm = np.stack([nx / ln, 1.0 / ln, nz / ln, np.zeros_like(x)], axis=-1)
    return pos, nrm, jx, jz


def eval_waves(S: Surface, t: float, xz: np.ndarray, **mistake):
    """ocean_eval_waves in float64 at the fp32 rest points xz [points, 2]: (pos, nrm, per-cascade sums)."""
    xz = np.asarray(xz, dtype=f32).reshape(-1, 2)
    double_wt = mistake.pop("double_wt", False)
    per = []
    for c, rows in enumerate(S.sets):
        tt = f32(t) + f32(S.toffs[c])
        fX = tile_fraction(xz[:, 0], S.n, S.grid, S.vd, S.scales[c])
        fZ = tile_fraction(xz[:, 1], S.n, S.grid, S.vd, S.scales[c])
        per.append(sums(rows, coefficients(rows, tt, double_wt), fX, fZ, **mistake))
    pos, nrm, _, _ = combine(S, per, xz[:, 0], xz[:, 1])
    return pos, nrm, per


def query_waves(S: Surface, t: float, xz: np.ndarray, iterations: int = 8):
    """ocean_query_waves as a float64 Newton iteration (the rest points are float64 throughout): (pos, nrm) with nrm[:, 3] the residual."""
    q = np.asarray(xz, dtype=f32).reshape(-1, 2).astype(np.float64)
    coef = [coefficients(rows, f32(t) + f32(S.toffs[c])) for c, rows in enumerate(S.sets)]

    def at(r):
        per = [sums(rows, coef[c], tile_fraction64(r[:, 0], S.n, S.grid, S.vd, S.scales[c]),
                    tile_fraction64(r[:, 1], S.n, S.grid, S.vd, S.scales[c])) for c, rows in enumerate(S.sets)]
        return combine(S, per, r[:, 0], r[:, 1])

    def clamp(j):
        return np.where(np.abs(j) < 0.1, np.where(j < 0.0, -0.1, 0.1), j)

    r = q.copy()
    for _ in range(iterations if iterations else 8):
        pos, _, jx, jz = at(r)
        r = np.stack([r[:, 0] - (pos[:, 0] - q[:, 0]) / clamp(jx), r[:, 1] - (pos[:, 2] - q[:, 1]) / clamp(jz)], axis=-1)
    pos, nrm, _, _ = at(r)
    nrm[:, 3] = np.hypot(pos[:, 0] - q[:, 0], pos[:, 2] - q[:, 1])
    return pos, nrm


# ------------------------------------------------------------------------------------------------------------------------------------
# the bound

def amplitudes(rows: np.ndarray) -> np.ndarray:
    """a_j = 2 (|re| + |im|) >= |c_j(t)| for every t."""
    return 2.0 * (np.abs(rows["re"].astype(np.float64)) + np.abs(rows["im"].astype(np.float64)))


def weights(rows: np.ndarray) -> np.ndarray:
    """g_j per channel of CHANNELS: 1, |ux|, |uz|, |kx|, |kz|, |kx ux|, |kz uz| -- [7, K]."""
    kx, kz, ux, uz = (np.abs(rows[k].astype(np.float64)) for k in ("kx", "kz", "ux", "uz"))
    return np.stack([np.ones_like(kx), ux, uz, kx, kz, kx * ux, kz * uz])


def sum_bound(rows: np.ndarray) -> np.ndarray:
    """Bound on |device sum - float64 sum| for each of the seven sums of ONE wave set of K rows, [7]:

        2^-21 * sum_j a_j g_j (|jx_j| + |jz_j| + 4 + K/8)

    Derivation, per wave j and channel with weight g (eps = 2^-24, the unit roundoff of fp32; the device's contribution is
    (g c)_fp32 * trig(2 pi ph_fp32), accumulated by fused multiply-adds):
      phase        fX, fZ are the same fp32 numbers on both sides.  a = (float)jx * fX is rounded once: |jx| eps turns at most; a - floor(a)
                   is exact or, for a tiny negative a, off by less than eps; the same for b; their sum (< 2) is rounded once: 2 eps.
                   Together (|jx| + |jz| + 2) eps turns = 2 pi (|jx| + |jz| + 2) eps radians, and sine and cosine have slope <= 1:
                   a g (|jx| + |jz| + 2) * 2 pi * 2^-24  <  0.79 * 2^-21 a g (|jx| + |jz| + 2).
      sine/cosine  the quarter turn is removed exactly (q / 4 and ph share their exponent range, the FMA is exact); the angle
                   x = 2 pi r with 2 pi in two floats: eps |x| <= 0.79 eps; the Cephes polynomials on [-pi/4, pi/4]: below 2 eps.
                   Below 2^-22 = 0.5 * 2^-21 per unit of a g.
      coefficient  the device's sincos_f32 is within 9e-8 of the true sine and cosine (its comment; the library path beyond 1e5 rad is
                   better), the reference's are correctly rounded (eps / 2); the two products, the difference and the doubling round as on
                   the reference but from those inputs: |c_dev - c_ref| <= 2 (|re| + |im|) (9e-8 + eps) < 1.6e-7 a < 0.34 * 2^-21 a.
      amplitude    g c for the channel is one or two more fp32 products (ux c; (kx ux) c): 2 eps = 0.25 * 2^-21 per unit of a g.
      together     0.79 (|jx| + |jz| + 2) + 0.5 + 0.34 + 0.25  <  |jx| + |jz| + 4                                  (per unit of 2^-21 a g)
      accumulation every FMA rounds a partial sum that is at most sum_j a_j g_j: K eps sum a g = (K / 8) 2^-21 sum a g.
    The GPU tests allow twice this."""
    k = len(rows)
    a = amplitudes(rows)
    j = np.abs(rows["jx"].astype(np.float64)) + np.abs(rows["jz"].astype(np.float64))
    return 2.0 ** -21 * (weights(rows) * (a * (j + 4.0 + k / 8.0))[None, :]).sum(axis=1)


def sum_max(rows: np.ndarray) -> np.ndarray:
    """The largest magnitude each of the seven sums can reach: sum_j a_j g_j, [7]."""
    return (weights(rows) * amplitudes(rows)[None, :]).sum(axis=1)


def bound(S: Surface, xmax: float = 0.0, zmax: float = 0.0):
    """Bound per OUTPUT channel of ocean_eval_waves against eval_waves above: (pos[4], nrm[4]).  From sum_bound per cascade, plus what the
    combination adds in fp32 (eps = 2^-24 per rounded operation, applied to the largest value the operand can take):
      pos.y   sum_c B_h,c + (C + 1) eps H,  H = sum_c sum a                         (C additions, the 0.0f + is exact)
      pos.x   sum_c |lam_c| B_dx,c + 2 C eps DX + eps (xmax + DX),  DX = sum_c |lam_c| sum a |ux|    (lam * Dx and its addition per
              cascade, then x + ...: the result is an fp32 number near x, which alone costs eps |x| -- xmax is the caller's largest |x|)
      pos.w   max over c of  |lam| (B_xx (1 + |lam| ZZ) + B_zz (1 + |lam| XX)) + lam^2 B_xx B_zz + 4 eps (1 + |lam| XX)(1 + |lam| ZZ)
              (|min_c a_c - min_c b_c| <= max_c |a_c - b_c|)
      normal  needs m = 1 - |choppy| sum_c XX_c >= 0.5 (and the same for ZZ): the tests assert it.  With SX the largest |S.x| and dsx, dxx
              the summed bounds (each + C eps of its maximum for the additions):
                d(nx) <= (dsx + eps SX) / m + SX (|choppy| dxx + 2 eps (1 + |choppy| XX)) / m^2 + eps SX / m
              and v -> v / |v| is 1-Lipschitz for |v| >= 1, so each component moves by at most d(nx) + d(nz), plus 4 eps for the square
              root and the three quotients.  nrm.w of the forward evaluation is exactly 0."""
    eps = 2.0 ** -24
    C = len(S.sets)
    B = np.array([sum_bound(r) for r in S.sets])        # [C, 7]
    M = np.array([sum_max(r) for r in S.sets])
    lam = np.abs(np.array(S.lams))
    ch = abs(S.choppy)
    H = M[:, 0].sum()
    pos_y = B[:, 0].sum() + (C + 1) * eps * H
    DX, DZ = (lam * M[:, 1]).sum(), (lam * M[:, 2]).sum()
    pos_x = (lam * B[:, 1]).sum() + 2 * C * eps * DX + eps * (xmax + DX)
    pos_z = (lam * B[:, 2]).sum() + 2 * C * eps * DZ + eps * (zmax + DZ)
    pos_w = max(lam[c] * (B[c, 5] * (1 + lam[c] * M[c, 6]) + B[c, 6] * (1 + lam[c] * M[c, 5])) + lam[c] ** 2 * B[c, 5] * B[c, 6]
                + 4 * eps * (1 + lam[c] * M[c, 5]) * (1 + lam[c] * M[c, 6]) for c in range(C))
    d = B.sum(axis=0) + C * eps * M.sum(axis=0)         # the summed S channels, [7]
    T = M.sum(axis=0)

    def raw(slope, dd):
        m = 1.0 - ch * T[dd]
        if m < 0.5:
            return np.inf
        return (d[slope] + eps * T[slope]) / m + T[slope] * (ch * d[dd] + 2 * eps * (1 + ch * T[dd])) / m ** 2 + eps * T[slope] / m

    n_b = raw(3, 5) + raw(4, 6) + 4 * eps
    return np.array([pos_x, pos_y, pos_z, pos_w]), np.array([n_b, n_b, n_b, 0.0])


def steepness(S: Surface) -> float:
    """G = rho = sum over every cascade and wave of a |k| (|lam| folded in where it exceeds 1): the Lipschitz constant of the height in the
    rest point and the contraction bound of the displacement, what the inverse's comparison divides by."""
    g = 0.0
    for c, rows in enumerate(S.sets):
        k = np.hypot(rows["kx"].astype(np.float64), rows["kz"].astype(np.float64))
        unit = S.scales[c] * S.lengths[c] / (S.grid * S.vd)       # ocean metres of tile c per mesh metre
        g += max(1.0, abs(S.lams[c])) * abs(unit) * float((amplitudes(rows) * k).sum())
    return g


# ------------------------------------------------------------------------------------------------------------------------------------
# points

def texel_centres(n: int, grid: int, vd: float) -> np.ndarray:
    """Rest points whose (u, v) at uv scale 1 and grid_size = N are the texel centres (n + 0.5) / N: [N * N, 2] fp32, row m = z."""
    assert grid == n
    c = ((np.arange(n, dtype=np.float64) + 0.5 - n // 2) * float(f32(vd))).astype(f32)
    return np.stack(np.meshgrid(c, c), axis=-1).reshape(-1, 2).astype(f32)
