"""Plain restatements of the two half-precision conversions on the device (helper module of tests/test_half_maps.py,
tests/test_zy_gather_half_gpu.py and tests/test_fp16_spectrum_gpu.py).

  pack_half      float32 -> IEEE half bits, round to nearest even, through numpy's cast: the reference for k_pack_half, the kernel behind
                 ocean_gather_maps_f16 (one RGBA32F texel -> four halves);
  rne_bits       the same conversion in integer arithmetic only, so that the reference is checked by something that is not numpy's cast;
  boundary_table every float32 value at which that conversion can go wrong: each finite half, the midpoint to its successor (a tie), the
                 float32 neighbours of the midpoint, the negatives, and the ends of both formats;
  quantise_h0    the fp16 copy of a tile's spectrum as the z pass reads it back (k_h0_absmax, k_h0_to_half, zpass_load_pair):
                 float(half(h0 * 2^(14 - e))) * 2^(e - 14), e the binary exponent of the tile's largest |component|.
"""
import numpy as np

F = np.float32
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)
HALF_MAX = 65504.0
FINITE_HALVES = 0x7c00            # bit patterns 0x0000 .. 0x7bff


def pack_half(a) -> np.ndarray:
    """uint16 bits of the halves nearest to the float32 array a (ties to even, beyond 65520 to +-inf)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    with np.errstate(over="ignore"):
        return a.astype(np.float16).view(np.uint16)


def rne_bits(a) -> np.ndarray:
    """pack_half without a floating-point cast: sign, 24-bit significand, a right shift by 13 (more for half subnormals), tie to even,
    the carry running into the exponent field; 0x7c00 and beyond is inf; a NaN becomes a quiet NaN of its sign."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.int64)
    sign = (u >> 16) & 0x8000
    exp = (u >> 23) & 0xff
    man = u & 0x7fffff
    sig = man | np.where(exp > 0, 1 << 23, 0)              # value = sig * 2^(E - 23)
    E = np.maximum(exp, 1) - 127
    shift = np.minimum(13 + np.maximum(0, -14 - E), 40)    # (beyond 25 everything rounds to zero: 40 keeps the masks inside int64)
    q = sig >> shift
    rem = sig & ((np.int64(1) << shift) - 1)
    half = np.int64(1) << (shift - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    # a normal half: q holds the hidden bit (1 << 10), so (E + 14) << 10 plus q is exponent field E + 15 with the mantissa below it
    bits = np.where(E >= -14, (E + 14) << 10, 0) + q
    bits = np.minimum(bits, 0x7c00)
    bits = np.where((exp == 255) & (man != 0), 0x7e00, bits)
    return (sign | bits).astype(np.uint16)


def _half_values():
    """(h, successor) as float64 for every finite non-negative half; the successor of 65504 is 65536."""
    h = np.arange(FINITE_HALVES, dtype=np.uint16).view(np.float16).astype(np.float64)
    return h, np.append(h[1:], 65536.0)


def midpoints() -> np.ndarray:
    """The float64 midpoint between every finite non-negative half and its successor (the last one is 65520)."""
    h, s = _half_values()
    return 0.5 * (h + s)


def boundary_table() -> np.ndarray:
    """float32: for every finite non-negative half h -- h, the midpoint to its successor, the float32 values one ulp under and over the
    midpoint -- then the negatives of all of these, then the ends: +-0, the smallest float32 denormal and normal, 2^-25 (the tie between
    0 and the smallest half) and its float32 successor, 65504, the float32 under 65520, 65520, 1e10, FLT_MAX, +-inf."""
    h, _ = _half_values()
    mid = midpoints().astype(np.float32)
    under, over = np.nextafter(mid, F(-np.inf)), np.nextafter(mid, F(np.inf))
    pos = np.stack([h.astype(np.float32), mid, under, over], axis=1).reshape(-1)
    tie0 = F(2.0 ** -25)
    extras = np.array([0.0, -0.0, 1e-45, -1e-45, FLT_MIN, tie0, np.nextafter(tie0, F(1.0)), HALF_MAX, np.nextafter(F(65520.0), F(0.0)),
                       65520.0, 1e10, FLT_MAX, np.inf, -np.inf], dtype=np.float32)
    return np.concatenate([pos, -pos, extras])


def padded_table(count: int, fill: float = 1.0) -> np.ndarray:
    """boundary_table() followed by `fill` up to count float32 values."""
    t = boundary_table()
    assert t.size <= count
    return np.concatenate([t, np.full(count - t.size, fill, np.float32)])


def h0_exponent(h0) -> int:
    """e of frexp(max |component|) = f * 2^e, f in [0.5, 1); 0 for a tile that is zero everywhere."""
    m = F(np.abs(np.asarray(h0, dtype=np.float32)).max())
    if m == 0:
        return 0
    return int(np.frexp(m)[1])


def quantise_h0(h0) -> np.ndarray:
    """The spectrum a frame with the fp16 copy really transforms, for ONE tile (any shape [..., 2] or complex pairs as the last axis):
    scale by the power of two that puts the tile's largest |component| into [2^13, 2^14), round to half (nearest even), widen, scale back.
    Every step in float32, and every product exact but the rounding to half."""
    h0 = np.ascontiguousarray(h0, dtype=np.float32)
    e = h0_exponent(h0)
    scale, inv = F(2.0 ** (14 - e)), F(2.0 ** (e - 14))
    with np.errstate(over="ignore", under="ignore"):
        return ((h0 * scale).astype(np.float32).astype(np.float16).astype(np.float32) * inv).astype(np.float32)
