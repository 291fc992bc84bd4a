"""CPU suite: the float32 statement of albedo demodulation (tests/np_albedo.py; include/mi_denoise.h, section a4k) held to answers
worked out by hand, so that the GPU tests compare the kernels with a checker that is itself checked."""
from fractions import Fraction

import numpy as np

import np_albedo as chk
import oracle


def px(r, g, b, a, dtype=np.float32):
    return np.array([[[r, g, b, a]]], dtype)


def test_a_quarter_over_a_half_is_a_half():
    out = chk.demodulate(px(0.25, 0.25, 0.25, 0.75), px(0.5, 0.5, 0.5, 0.125))
    assert out.dtype == np.float32 and np.array_equal(out, px(0.5, 0.5, 0.5, 0.75))
    back = chk.modulate(out, px(0.5, 0.5, 0.5, 0.125))
    assert np.array_equal(back, px(0.25, 0.25, 0.25, 0.75))


def test_zero_nan_and_negative_albedo_divide_by_the_floor():
    floor = np.float32(1e-3)
    want = np.float32(0.25) / floor
    for a in (0.0, -0.0, np.nan, -1.0, -np.inf, 1e-42, 1e-3):       # (a subnormal and the floor itself too)
        out = chk.demodulate(px(0.25, 0.25, 0.25, 1.0), px(a, a, a, a), floor)
        assert np.array_equal(out[0, 0, :3], np.full(3, want, np.float32)) and out[0, 0, 3] == 1.0, a
        back = chk.modulate(out, px(a, a, a, a), floor)
        assert np.array_equal(back[0, 0, :3], np.full(3, want * floor, np.float32)), a
    other = chk.demodulate(px(0.25, 0.25, 0.25, 1.0), px(0.0, 0.0, 0.0, 1.0), 0.5)
    assert np.array_equal(other[0, 0, :3], np.full(3, 0.5, np.float32))                # the floor is a parameter


def test_an_infinite_albedo_gives_zero_and_then_nan():
    out = chk.demodulate(px(0.25, 2.0, 1e4, 1.0), px(np.inf, np.inf, np.inf, 1.0))
    assert np.array_equal(out, px(0.0, 0.0, 0.0, 1.0))
    back = chk.modulate(out, px(np.inf, np.inf, np.inf, 1.0))
    assert np.isnan(back[0, 0, :3]).all() and back[0, 0, 3] == 1.0


def test_every_u8_code_widens_to_the_correctly_rounded_quotient():
    codes = np.arange(256, dtype=np.uint8).reshape(1, 64, 4)
    got = chk.widen(codes).reshape(-1)
    assert got.dtype == np.float32
    for c in range(256):
        exact, g = Fraction(c, 255), got[c]
        err = abs(Fraction(float(g)) - exact)
        for nb in (np.nextafter(g, np.float32(-1)), np.nextafter(g, np.float32(2))):
            assert err <= abs(Fraction(float(nb)) - exact), c
    a = chk.demodulate(px(1.0, 1.0, 1.0, 1.0), px(128, 128, 128, 7, np.uint8))
    q = np.float32(128.0) / np.float32(255.0)
    assert q == np.float32(0.5019608) and np.array_equal(a[0, 0, :3], np.full(3, np.float32(1.0) / q, np.float32))
    f = chk.demodulate(px(128, 0, 255, 255, np.uint8), px(1.0, 1.0, 1.0, 1.0))           # a u8 frame widens the same way
    assert np.array_equal(f, px(q, 0.0, 1.0, 1.0))


def test_alpha_is_untouched_and_the_albedo_alpha_is_ignored():
    rng = np.random.default_rng(3)
    fr = rng.random((5, 7, 4), dtype=np.float32)
    al = rng.random((5, 7, 4), dtype=np.float32)
    fr[0, 0, 3], fr[1, 1, 3] = np.nan, np.inf
    al2 = al.copy()
    al2[..., 3] = 0.0
    d = chk.demodulate(fr, al)
    assert np.array_equal(d[..., 3].view(np.uint32), fr[..., 3].view(np.uint32))
    assert np.array_equal(d.view(np.uint32), chk.demodulate(fr, al2).view(np.uint32))
    m = chk.modulate(d, al)
    assert np.array_equal(m[..., 3].view(np.uint32), fr[..., 3].view(np.uint32))
    h = chk.demodulate(fr.astype(np.float16), al.astype(np.float16))
    assert np.array_equal(h[..., 3].view(np.uint32), fr.astype(np.float16).astype(np.float32)[..., 3].view(np.uint32))


def test_u8_output_truncates_and_f16_rounds_to_nearest_even():
    one = px(1.0, 1.0, 1.0, 1.0)
    # 255 * x is truncated: 0.999 -> 254, 1.0 -> 255, 0.5 -> 127; outside the cast's domain it clamps, NaN gives 0
    got = chk.modulate(px(0.999, 1.0, 0.5, 2.0), one, out_dtype=np.uint8)
    assert got.dtype == np.uint8 and got[0, 0].tolist() == [254, 255, 127, 255]
    got = chk.modulate(px(-0.003, -1.0, np.nan, 1.0039), one, out_dtype=np.uint8)
    assert got[0, 0].tolist() == [0, 0, 0, 255]
    rng = np.random.default_rng(4)
    x = (rng.random((16, 16, 4), dtype=np.float32) * 1.2 - 0.1).astype(np.float32)
    assert np.array_equal(chk.pack_u8(x), oracle.pack_u8(x))
    # binary16 has 10 fraction bits: 1 + 2^-11 is a tie and goes to the even 1.0, 1 + 3 * 2^-11 to the even 1 + 2^-9
    got = chk.modulate(px(1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -20, 70000.0), one, out_dtype=np.float16)
    assert got.dtype == np.float16
    assert got[0, 0, 0] == np.float16(1.0) and got[0, 0, 1] == np.float16(1 + 2.0 ** -9) and got[0, 0, 2] == np.float16(1 + 2.0 ** -10)
    assert np.isposinf(got[0, 0, 3])
    # the product is rounded to float32 first, then packed
    got = chk.modulate(px(0.5, 0.5, 0.5, 1.0), px(0.999, 0.999, 0.999, 1.0), out_dtype=np.uint8)
    assert got[0, 0, 0] == int(np.float32(255.0) * (np.float32(0.5) * np.float32(0.999)))


def test_the_round_trip_is_within_two_roundings():
    rng = np.random.default_rng(5)
    c = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), (64, 64, 4))).astype(np.float32)
    a = np.exp(rng.uniform(np.log(1e-3), np.log(1.0), (64, 64, 4))).astype(np.float32)
    back = chk.modulate(chk.demodulate(c, a), a)
    err = np.abs(back.astype(np.float64) - c.astype(np.float64))
    assert (err <= 2.0 ** -22 * np.abs(c.astype(np.float64))).all()
    assert (err > 0).any()                                                          # (it is not an identity)
    # below the floor both passes use the floor: the round trip still holds, the illumination is C / floor
    z = np.zeros_like(a)
    back = chk.modulate(chk.demodulate(c, z), z)
    assert (np.abs(back.astype(np.float64) - c) <= 2.0 ** -22 * np.abs(c.astype(np.float64))).all()
