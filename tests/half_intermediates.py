"""Float64 restatement of a frame with half2 intermediates (ocean_set_intermediate_precision(16): the Z16 instantiation of every frame
kernel; helper module of tests/test_half_intermediates.py and tests/test_half_intermediates_gpu.py).

Between the two passes that mode stores the z-pass outputs as halves: every packed pair of DESIGN.md section 2 (and the height's real
transform) is transformed along kz, the real and the imaginary part of every element are multiplied by a per-tile power of two, rounded
to nearest even, and the x pass divides the power of two out again.  Everything else of the frame is the fp32 path.  So the float64
two-pass transform that rounds at the same place to the same halves is what such a frame is meant to compute, and the distance between
a frame and it is the kernels' own fp32 noise plus the few halves that noise rounds the other way -- far less than the distance of
either from the unquantised oracle, which is the rounding itself.

  bound_scales  the host rule of ocean_prepare ("scales of the half2 intermediates") on two given bounds;
  scales        k_inter_bounds + that rule on a spectrum, with the distance of every choice from the next power of two;
  frame         the frame (A, displacement map, normal map, min, max) as oracle.numpy_compute_waves returns it;
  frame_pair    the restated and the unquantised frame off the same first-axis transforms (large tiles);
  ratios        rms and max of (gpu - restated) over those of (restated - oracle), per channel.

numpy and scipy only; float64 but for the fp32 products and the halves that are the library's own arithmetic.
"""
from __future__ import annotations

import os

import numpy as np

F = np.float32
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)
HALF_TOP = 32768.0          # the rule aims the bound of a stored component at 2^15; the largest finite half is 65504
WORKERS = min(16, os.cpu_count() or 1)


# --------------------------------------------------------------------------------------------------------------------------------
# scales

def pow2_below(x: float) -> float:
    """The largest power of two <= x (x > 0, finite)."""
    f, e = np.frexp(x)                  # x = f * 2^e, f in [0.5, 1)
    return float(np.ldexp(1.0, int(e) - 1))


def pow2_distance(x: float) -> float:
    """How far x > 0 is from the nearest power of two, relative to that power: 0 on a power of two, at most 1/3 (reached at
    x = 4/3 * 2^e, which is as far from 2^e as from 2^(e+1) in this measure); inf where there is no x to speak of."""
    if not (x > 0.0 and np.isfinite(x)):
        return float("inf")
    f, _ = np.frexp(x)
    return float(min(2.0 * f - 1.0, 1.0 - f))          # (x - 2^(e-1)) / 2^(e-1), (2^e - x) / 2^e


def _scale_for(bound4: float):
    """(scale, pow2_distance of the quotient it is taken from) for a stored component bounded by bound4."""
    if not (bound4 > 0.0 and np.isfinite(bound4)):
        return 1.0, float("inf")
    x = HALF_TOP / bound4
    return pow2_below(x), pow2_distance(x)


def bound_scales(b0: float, b1: float) -> dict:
    """The scales of one tile from its two bounds -- b0 the largest column sum of |h0|, b1 of |k| |h0|: a stored component is at most
    2 (column sum + mirrored column sum) <= 4 bound, and the scale is the largest power of two that keeps 4 bound scale <= 32768.
    su: pair 0 and the height; sk: pairs 1 and 2; g: the power of two that lifts pair 3's cross derivative to the height's magnitude,
    the largest one <= b0 / b1; s3: pair 3, from 4 (b0 + g b1).  A bound that is zero, inf or NaN gives 1.
    "distance": pow2_distance of the quotient behind each choice (inf where the choice is the constant 1)."""
    b0, b1 = float(b0), float(b1)
    su, du = _scale_for(4.0 * b0)
    sk, dk = _scale_for(4.0 * b1)
    with np.errstate(all="ignore"):
        r = np.float64(b0) / np.float64(b1) if (b0 > 0.0 and b1 > 0.0) else np.float64("nan")
    if b0 > 0.0 and b1 > 0.0 and np.isfinite(r) and r > 0.0:
        g, dg = pow2_below(float(r)), pow2_distance(float(r))
    else:
        g, dg = 1.0, float("inf")
    with np.errstate(all="ignore"):
        s3, d3 = _scale_for(float(4.0 * (np.float64(b0) + np.float64(g) * np.float64(b1))))
    return dict(su=su, sk=sk, g=g, s3=s3, b0=b0, b1=b1, distance=dict(su=du, sk=dk, g=dg, s3=d3))


def scales(h0, kx, kz) -> dict:
    """bound_scales of a spectrum.  h0 complex [m, q] (row m: kz, column q: kx, as oracle.numpy_prepare), kx and kz the fp32 wave
    numbers of the same shape.  The bounds are the sums of |h0| and of |k| |h0| over each spectrum column -- a fixed kx: down axis 0
    -- and their maxima over the columns.  The device sums in fp32 in an order of its own; this sums in float64.  The two can pick
    different powers of two only where the quotient is within a few 1e-7 of one, hence "distance": callers assert that it is far
    larger (1e-3) for their inputs, and then this IS the device's choice."""
    h0 = np.asarray(h0)
    mag = np.hypot(h0.real.astype(np.float64), h0.imag.astype(np.float64))
    k = np.hypot(np.asarray(kx, np.float64), np.asarray(kz, np.float64))
    with np.errstate(all="ignore"):
        b0 = float(mag.sum(axis=0).max())
        b1 = float((mag * k).sum(axis=0).max())
    return bound_scales(b0, b1)


# --------------------------------------------------------------------------------------------------------------------------------
# the rounding

def to_half(x: np.ndarray, rounding: str = "rne") -> np.ndarray:
    """float64 -> the half the device stores, as float64: through float32 (the kernel's product v * scale is a float, and exact: the
    scale is a power of two) to float16, round to nearest even, subnormals kept, beyond 65520 inf.  rounding="rz" rounds toward zero
    instead (no kernel does; it is the mutation tests/test_half_intermediates.py measures the criterion on)."""
    with np.errstate(over="ignore", under="ignore"):
        x32 = np.asarray(x, np.float64).astype(np.float32)
        h = x32.astype(np.float16)
        if rounding == "rz":
            over = np.abs(h.astype(np.float32)) > np.abs(x32)               # (inf too: back to 65504)
            h = np.where(over, np.nextafter(h, np.float16(0.0)), h)
        elif rounding != "rne":
            raise ValueError(rounding)
        return h.astype(np.float64)


class _Quantiser:
    """Scale, round, unscale of one stored array; remembers the largest scaled magnitude it saw."""

    def __init__(self, rounding="rne", noise=0.0, seed=0):
        self.rounding, self.noise = rounding, float(noise)
        self.rng = np.random.default_rng(seed)
        self.max_scaled = 0.0

    def __call__(self, y: np.ndarray, scale: float) -> np.ndarray:
        if self.noise:
            # a stand-in for the fp32 z pass: both parts of every element move by a gaussian of `noise` times the rms of their column
            rms = np.sqrt(np.mean(np.abs(y) ** 2, axis=0, keepdims=True))
            y = y + self.noise * rms * (self.rng.standard_normal(y.shape) + 1j * self.rng.standard_normal(y.shape))
        re, im = y.real * scale, y.imag * scale
        self.max_scaled = max(self.max_scaled, float(np.abs(re).max()), float(np.abs(im).max()))
        return (to_half(re, self.rounding) + 1j * to_half(im, self.rounding)) / scale


# --------------------------------------------------------------------------------------------------------------------------------
# the frame

def _mirror(x: np.ndarray) -> np.ndarray:
    """x(-m, -q): both indices negated modulo N."""
    return np.roll(x[::-1, ::-1], 1, axis=(0, 1))


def _animate(prep, t):
    """h~ = 2 (Re h0 cos wt - Im h0 sin wt), exactly as oracle.numpy_compute_waves: ONE fp32 product w t, then sincos."""
    wt = (prep["omega"] * F(t)).astype(F)
    c, s = np.cos(wt.astype(np.float64)).astype(F), np.sin(wt.astype(np.float64)).astype(F)
    h0 = prep["h0"]
    return (F(2.0) * ((h0.real * c).astype(F) - (h0.imag * s).astype(F)).astype(F)).astype(np.float64)


def _frames(prep, t, lam, jacobian, quantisers, info=None):
    """One frame per entry of `quantisers` (a _Quantiser, or None for the plain two-pass transform), all off the same first-axis
    transforms."""
    import scipy.fft as sfft
    n = prep["kx"].shape[0]
    hr = _animate(prep, t)
    kx, kz, ux, uz = (prep[k].astype(np.float64) for k in ("kx", "kz", "ux", "uz"))
    sc = scales(prep["h0"], prep["kx"], prep["kz"])
    if info is not None:
        info["scales"] = sc
    sign = 1.0 - 2.0 * ((np.arange(n)[:, None] + np.arange(n)[None, :]) & 1)

    def two_pass(packed, scale):
        """S Re and S Im of the backward transform of `packed`, kz first, the intermediate rounded by each quantiser."""
        y = sfft.ifft(packed, axis=0, norm="forward", workers=WORKERS)      # a spectrum column (fixed kx) is transformed first
        out = []
        for q in quantisers:
            z = sfft.ifft(y if q is None else q(y, scale), axis=1, norm="forward", workers=WORKERS)
            out.append((sign * z.real, sign * z.imag))
        return out

    g = sc["g"]
    hm = _mirror(hr)
    kxm, kzm, uxm, uzm = (_mirror(a) for a in (kx, kz, ux, uz))                 # (k(-idx) = -k(idx) but on the Nyquist lines, index 0)

    # The Hermitian part (X(idx) + conj X(-idx)) / 2 of X = c h~ (Re B[X] = B[X_h]) for a real coefficient r, r(-idx) = rm, and
    # for an imaginary one, c = i r, where it is i times the value returned: both in real arithmetic.
    def herm_re(r, rm):
        return 0.5 * (r * hr + rm * hm)

    def herm_im(r, rm):
        return 0.5 * (r * hr - rm * hm)

    def packed(re, im):
        out = np.empty(hr.shape, np.complex128)
        out.real, out.imag = re, im
        return out

    # the packed pairs of DESIGN.md section 2, each part the Hermitian part of c_f h~; with A, B the real arrays behind two imaginary
    # parts i A and i B, the pair i A + i (i B) is (-B, A)
    pair0 = two_pass(packed(-herm_im(-uz, -uzm), herm_im(-ux, -uxm)), sc["su"])                     # Dx + i Dz, c = -i ux, -i uz
    pair1 = two_pass(packed(-herm_im(kz, kzm), herm_im(kx, kxm)), sc["sk"])                          # sx + i sz, c = i kx, i kz
    pair2 = two_pass(packed(herm_re(kx * ux, kxm * uxm), herm_re(kz * uz, kzm * uzm)), sc["sk"])     # dxDx + i dzDz
    splus = 0.5 * (hr + hm)
    if jacobian:                                                                                     # h + i g dxDz, one scale
        # ONE cross derivative, kx kz / |k|, serves as dxDz and as dzDx; with the fp32 unit vectors of `prep`, kx uz and kz ux are two
        # roundings of it, 1e-7 apart, and their mean squared is the oracle's product dxDz dzDx to 1e-14
        pair3 = two_pass(packed(splus, g * herm_re(0.5 * (kx * uz + kz * ux), 0.5 * (kxm * uzm + kzm * uxm))), sc["s3"])
    else:                                                                                            # the real height S+
        pair3 = two_pass(packed(splus, 0.0), sc["su"])
    frames = []
    for i in range(len(quantisers)):
        (dx, dz), (sx, sz), (dxdx, dzdz), (h, cross) = pair0[i], pair1[i], pair2[i], pair3[i]
        hmin = min(float(h.min()), FLT_MAX)
        hmax = max(float(h.max()), FLT_MIN)                                 # the running maximum starts at FLT_MIN (.cpp:289)
        amp = max(abs(hmin), abs(hmax))
        w = np.ones_like(h)
        if jacobian:
            dxdz = cross / g                                                # dzDx is the same field
            w = (1.0 + lam * dxdx) * (1.0 + lam * dzdz) - (lam * dxdz) * (lam * dxdz)
        frames.append((amp, np.stack([lam * dx, h / amp, lam * dz, w], axis=-1), np.stack([sx, sz, dxdx, dzdz], axis=-1), hmin, hmax))
    if info is not None:
        info["max_scaled"] = max((q.max_scaled for q in quantisers if q is not None), default=0.0)
    return frames


def frame(prep, t, lam=-1.0, jacobian=False, quantise=True, rounding="rne", noise=0.0, seed=0, info=None):
    """(A, disp[n, n, 4], nrm[n, n, 4], min, max) of one frame with half2 intermediates, like oracle.numpy_compute_waves.

    prep: oracle.numpy_prepare's dictionary, so that h0 can be the device's own (read_spectrum), tests/half_maps.quantise_h0 of it or
    tests/empirical_spectra.restate_h0.  The Hermitian parts of the seven (Jacobian mode: eight) fields are packed as DESIGN.md section
    2 lists, transformed along kz (a spectrum column is a fixed kx: axis 0 of the [m, q] layout is what is transformed), both parts
    of every element multiplied by the scale of their array (scales: su for pair 0 and the height, sk for pairs 1 and 2, s3 for pair 3,
    whose cross derivative went in times g), rounded to half and divided by the scale again, transformed along kx, given the sign
    (-1)^(p+q); g is divided out, A, min and max come off the quantised height with the FLT_MIN quirk, and the maps and the Jacobian
    slot are formed as the oracle forms them.

    The device stores only half of the rows and columns and reads the rest back as +- conjugates.  Rounding to nearest (and toward
    zero) is odd and acts on the real and the imaginary part separately, so it commutes with both: quantising the full array, as done
    here, is the same thing.

    quantise=False: the same two passes without the rounding (equals numpy_compute_waves to rounding error).
    rounding="rz": toward zero.  noise: relative size of a gaussian added to the z-pass output before rounding (see _Quantiser).
    info: a dictionary that receives "scales" and "max_scaled", the largest |component| * scale that was rounded."""
    q = _Quantiser(rounding, noise, seed) if quantise else None
    return _frames(prep, t, lam, jacobian, [q], info)[0]


def frame_pair(prep, t, lam=-1.0, jacobian=False, info=None):
    """(restated frame, unquantised frame): frame(...) and frame(..., quantise=False) off one set of first-axis transforms, for
    tiles where the float64 transforms are what a test's time goes into."""
    restated, plain = _frames(prep, t, lam, jacobian, [_Quantiser(), None], info)
    return restated, plain


# --------------------------------------------------------------------------------------------------------------------------------
# the criterion

def channels(disp, nrm) -> list:
    """The eight channels of both maps as a list of [n, n] views (no copy: a 4096^2 frame is half a gigabyte per map in float64)."""
    return [disp[..., c] for c in range(4)] + [nrm[..., c] for c in range(4)]


def errors(a, b) -> list:
    """max|a - b| / max|b| per channel (lists as channels() returns them), in float64."""
    out = []
    for x, y in zip(a, b):
        y = np.asarray(y, np.float64)
        out.append(float(np.abs(np.asarray(x, np.float64) - y).max()) / max(float(np.abs(y).max()), 1e-30))
    return out


def ratios(gpu, restated, oracle):
    """Per channel (lists as channels() returns them): (rms(gpu - restated) / rms(restated - oracle), max|gpu - restated| /
    max|restated - oracle|).  A channel in which the restatement IS the oracle (the constant Jacobian slot of FULL7, a channel that is
    zero everywhere) has no rounding to compare with: None for both."""
    out = []
    for g, rs, o in zip(gpu, restated, oracle):
        rs = np.asarray(rs, np.float64)
        e, r = np.asarray(g, np.float64) - rs, rs - np.asarray(o, np.float64)
        if not r.any():
            out.append((None, None))
            continue
        out.append((float(np.sqrt(np.mean(e * e)) / np.sqrt(np.mean(r * r))), float(np.abs(e).max() / np.abs(r).max())))
    return out
