"""GPU suite: mid_color_bounds (section a4m) on frames whose answer is known exactly.

The frame is tiled with a (2 R + 1) x (2 R + 1) pattern of integers a + d dev[k], so the window of every interior pixel holds each
of the pattern's (2 R + 1)^2 texels exactly once, in an order that depends on the pixel -- and the answer does not:

    R = 1: dev = {-3, -3, 3, 3, 0, 0, 0, 0, 0}:            sum dev = 0, sum dev^2 = 36 = 9 x 2^2,   so mu = a and sigma = 2 d
    R = 2: dev = {-5, -5, 5, 5, 0 (21 times)}:             sum dev = 0, sum dev^2 = 100 = 25 x 2^2, so mu = a and sigma = 2 d

a and d are small multiples of 16 and gamma a power of two: every sum is a sum of small integers (exact in fp32 and in binary64, in
any order), the quotients 9 a / 9 and 36 d^2 / 9 are exact, sqrtf of the perfect square 4 d^2 is exact (IEEE: sqrtf is correctly
rounded -- the build uses no fast-math flag), and so is the fma.  Every interior pixel is therefore bit for bit a -+ gamma 2 d, in
every arrangement of the pattern inside its tile -- which pins the tap offsets: a kernel that reads a window one texel off, or
skips or repeats a tap, meets another multiset.  The three channels carry three different (a, d) and three different arrangements.
"""
import numpy as np
import pytest

from test_gpu_atrous_bounds import bits
from test_gpu_color_bounds import raw_bounds

pytestmark = pytest.mark.gpu

DEV = {1: [-3, -3, 3, 3] + [0] * 5, 2: [-5, -5, 5, 5] + [0] * 21}
AD = ((96, 16), (160, 16), (64, 0))                  # (a, d) per channel, a -+ 5 d inside 0..255; d = 0: a constant channel


def pattern_frame(shape, radius, dt, seed):
    h, w = shape
    k = 2 * radius + 1
    rng = np.random.default_rng([31, seed])
    yy, xx = np.mgrid[0:h, 0:w]
    chans = []
    for a, d in AD:
        tile = rng.permutation(np.array(DEV[radius]))[: k * k].reshape(k, k)          # any arrangement inside the tile
        chans.append(a + d * tile[yy % k, xx % k])
    chans.append(rng.integers(0, 256, (h, w)))
    fr = np.stack(chans, -1).astype(np.float64)
    assert fr.min() >= 0 and fr.max() <= 255
    return fr.astype(dt)


@pytest.mark.parametrize("dt", (np.float32, np.float16), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("radius", (1, 2))
def test_every_interior_pixel_is_a_minus_and_plus_gamma_2d(ctx, radius, dt):
    shape = (37, 133)                                    # three tile rows, three tile columns, both seams inside
    for seed in range(4):
        fr = pattern_frame(shape, radius, dt, seed)
        for gamma in (0.5, 1.0, 4.0):
            lo, hi = raw_bounds(ctx, fr, radius, gamma)
            inner = (slice(radius, shape[0] - radius), slice(radius, shape[1] - radius))
            for c, (a, d) in enumerate(AD):
                want_lo, want_hi = np.float32(a - gamma * 2 * d), np.float32(a + gamma * 2 * d)
                assert (bits(lo[inner + (c,)]) == bits(want_lo)).all() and (bits(hi[inner + (c,)]) == bits(want_hi)).all(), (radius, seed, gamma, c)
            assert (lo[inner + (3,)] == (2 * radius + 1) ** 2).all()
            assert not np.array_equal(lo[..., 0], np.full(shape, lo[radius, radius, 0])), "the cropped windows at the border hold another multiset"


def test_uint8_codes_up_to_their_roundings(ctx):
    """uint8 frames hold c / 255, not integers: the same patterns in codes give mu = a / 255 and sigma = 2 d / 255 up to the rounding
    of the 255ths -- the float64 checker's business (test_gpu_color_bounds.py); here only that every interior pixel of a channel has
    ONE value, whatever the arrangement, up to those roundings: every widened texel carries 2^-25 of itself, so does the mean, the
    deviations and with them sigma carry twice 2^-25 (a + 5 d) / 255, the fma rounds once more: below 5 x 2^-25 (a + 5 d) / 255, which
    16 x 2^-25 (a + 2 d) / 255 bounds."""
    for radius in (1, 2):
        fr = pattern_frame((37, 133), radius, np.uint8, 9)
        lo, hi = raw_bounds(ctx, fr, radius, 1.0)
        inner = (slice(radius, 37 - radius), slice(radius, 133 - radius))
        for c, (a, d) in enumerate(AD):
            for plane, want in ((lo, (a - 2 * d) / 255), (hi, (a + 2 * d) / 255)):
                v = plane[inner + (c,)].astype(np.float64)
                assert np.abs(v - want).max() <= 16 * 2.0 ** -25 * (a + 2 * d) / 255, (radius, c)
