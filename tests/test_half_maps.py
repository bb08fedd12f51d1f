"""tests/half_maps.py checked on the CPU: the reference of the f16 gather (numpy's float32 -> float16 cast) against the same conversion in
integer arithmetic on every rounding boundary, what the boundary table contains, and the restated fp16 spectrum's own properties."""
import numpy as np

import half_maps as H

F = np.float32


def test_numpy_cast_is_round_to_nearest_even_on_every_boundary():
    t = H.boundary_table()
    assert t.dtype == np.float32 and t.size == 4 * 2 * H.FINITE_HALVES + 14 == 253966
    assert t.size <= 256 * 256 * 4                                   # one 256^2 RGBA32F map holds it
    assert not np.isnan(t).any()
    got, want = H.pack_half(t), H.rne_bits(t)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad.size, t[bad[:4]], got[bad[:4]], want[bad[:4]])
    # a NaN is a NaN in both (numpy: 0x7e00), whatever its payload
    nan = np.array([np.nan, -np.nan], np.float32)
    nan = np.concatenate([nan, np.array([0x7f800001, 0xffc12345], np.uint32).view(np.float32)])
    for bits in (H.pack_half(nan), H.rne_bits(nan)):
        assert np.all((bits & 0x7c00) == 0x7c00) and np.all((bits & 0x03ff) != 0)
    assert H.pack_half(nan[:1])[0] == 0x7e00


def test_midpoints_are_float32_values_and_round_both_ways():
    mid = H.midpoints()
    assert mid.size == H.FINITE_HALVES and mid[-1] == 65520.0
    assert np.array_equal(mid.astype(np.float32).astype(np.float64), mid)          # exactly representable: the ties are real ties
    m32 = mid.astype(np.float32)
    lo = np.arange(H.FINITE_HALVES, dtype=np.int64)
    bits = H.pack_half(m32).astype(np.int64)
    up, down = bits == lo + 1, bits == lo
    assert np.all(up | down)
    assert np.array_equal(down, lo % 2 == 0)                                       # ties go to the even neighbour ...
    assert up.sum() == down.sum() == H.FINITE_HALVES // 2                          # ... half of them up, half of them down
    assert bits[-1] == 0x7c00                                                      # 65520 -> inf
    # one float32 ulp beside the tie decides it
    assert np.array_equal(H.pack_half(np.nextafter(m32, F(-np.inf))).astype(np.int64), lo)
    assert np.array_equal(H.pack_half(np.nextafter(m32, F(np.inf))).astype(np.int64), lo + 1)


def test_table_holds_subnormals_both_sides_of_65520_and_the_ends():
    t = H.boundary_table()
    bits = H.pack_half(t)
    mag = bits & 0x7fff
    sub = (mag > 0) & (mag < 0x0400)
    assert sub.sum() >= 2 * 4 * 1022 and (bits[sub] & 0x8000).any() and not (bits[sub] & 0x8000).all()     # half subnormals of both signs
    fin = np.isfinite(t)
    assert np.all(mag[fin & (np.abs(t) >= 65520.0)] == 0x7c00)                     # saturates to inf from 65520 on ...
    assert np.all(mag[np.abs(t) < 65520.0] < 0x7c00)                               # ... and not before
    just_under = np.nextafter(F(65520.0), F(0.0))
    for v, want in ((just_under, 0x7bff), (F(65520.0), 0x7c00), (F(-65520.0), 0xfc00), (-just_under, 0xfbff), (F(65504.0), 0x7bff),
                    (F(1e10), 0x7c00), (F(H.FLT_MAX), 0x7c00), (F(np.inf), 0x7c00), (F(-np.inf), 0xfc00)):
        at = np.nonzero(t == v)[0]
        assert at.size >= 1 and np.all(bits[at] == want), (v, want)
    # signed zeros, and what underflows to them: fp32 denormals, FLT_MIN, the tie 2^-25 (to even: 0); its successor is the smallest half
    z = t.view(np.uint32)
    assert bits[np.nonzero(z == 0x00000000)[0]].tolist() == [0, 0] and bits[np.nonzero(z == 0x80000000)[0]].tolist() == [0x8000, 0x8000]
    assert bits[np.nonzero(z == 0x00000001)[0]].tolist() == [0] and bits[np.nonzero(z == 0x80000001)[0]].tolist() == [0x8000]
    assert np.all(bits[t == F(H.FLT_MIN)] == 0)
    tie0 = F(2.0 ** -25)
    assert np.all(bits[t == tie0] == 0) and np.all(bits[t == np.nextafter(tie0, F(1.0))] == 1)
    p = H.padded_table(256 * 256 * 4)
    assert p.size == 262144 and np.array_equal(p[:t.size].view(np.uint32), z) and np.all(p[t.size:] == 1.0)


def test_quantised_spectrum_properties():
    rng = np.random.default_rng(16)
    for n, amp in ((16, 1.0), (64, 3.1e-4), (64, 7.7e3)):
        h0 = (rng.standard_normal((n, n, 2)) * amp * rng.uniform(1e-4, 1.0, (n, n, 1))).astype(np.float32)
        h0[n // 2, n // 2] = 0.0
        q = H.quantise_h0(h0)
        assert q.dtype == np.float32 and q.shape == h0.shape
        e = H.h0_exponent(h0)
        big = np.abs(h0).max() * F(2.0 ** (14 - e))
        assert 2.0 ** 13 <= big < 2.0 ** 14                                        # the largest component lands in [2^13, 2^14)
        # ... where halves are 8 apart: half a step of the largest component bounds every error
        assert np.abs(q.astype(np.float64) - h0).max() <= 4.0 * 2.0 ** (e - 14)
        assert np.array_equal(H.quantise_h0(q).view(np.uint32), q.view(np.uint32))  # idempotent
        assert not np.array_equal(q, h0) and np.all(q[n // 2, n // 2] == 0.0)
        assert np.array_equal(np.signbit(q), np.signbit(h0))                        # nothing changes sign, not even what rounds to zero
    # the scale is a power of two: scaling the tile by one scales the result by it, exactly
    assert np.array_equal(H.quantise_h0(h0 * F(2.0 ** -9)), H.quantise_h0(h0) * F(2.0 ** -9))
    # a component of exactly a power of two: frexp gives f = 0.5, so it lands on 2^13
    one = np.zeros((4, 4, 2), np.float32); one[1, 2, 0] = -0.25; one[0, 0, 1] = 0.25 * 2.0 ** -11 * (1 + 2.0 ** -11)
    assert H.h0_exponent(one) == -1 and np.array_equal(H.quantise_h0(one)[1, 2], [-0.25, 0.0])
    assert H.quantise_h0(one)[0, 0, 1] == F(0.25 * 2.0 ** -11)                     # 2^2 (1 + 2^-11) rounds down to the even half 4
    # a zero tile stays zero, signs and all
    zero = np.zeros((8, 8, 2), np.float32); zero[3, 3, 1] = -0.0
    assert H.h0_exponent(zero) == 0 and np.array_equal(H.quantise_h0(zero).view(np.uint32), zero.view(np.uint32))
