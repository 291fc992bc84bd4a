"""CPU suite: the float64 checker of the neighbourhood colour box (tests/np_color_bounds.py; include/mi_denoise.h, section a4m) against
a per-pixel loop that vectorises nothing, and against answers worked out by hand."""
import numpy as np
import pytest

from firefly_inputs import frame_of
from np_color_bounds import color_bounds, color_bounds_loop


@pytest.mark.parametrize("dt", (np.uint8, np.float16, np.float32), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("radius", (1, 2))
def test_the_checker_is_the_per_pixel_loop(radius, dt):
    """On frames with NaN, +-Inf and negative channels (the firefly recipe): the same windows, the same validity, the same sums."""
    for shape, gamma in (((1, 1), 1.0), ((2, 3), 0.0), ((9, 17), 2.5), ((16, 23), 1.0)):
        fr = frame_of(shape, dt, 3)
        if np.dtype(dt) != np.uint8:
            fr[fr > 100] = 100                       # (the recipe's 4096 x fireflies: kept, but inside float16's squares)
        got, want = color_bounds(fr, radius, gamma), color_bounds_loop(fr, radius, gamma)
        for g, w in zip(got, want):
            assert np.array_equal(np.isinf(g), np.isinf(w)) and not np.isnan(g).any()
            fin = np.isfinite(w)
            assert np.allclose(g[fin], w[fin], rtol=1e-12, atol=1e-12)
            assert np.array_equal(g[..., 3], w[..., 3])


def test_one_pixel_is_its_own_box():
    for dt, c in ((np.float32, [0.3, 7.5, 1e-3, 0.25]), (np.float16, [0.5, 2.0, 1024.0, 0.0]), (np.uint8, [0, 255, 77, 3])):
        fr = np.array(c, dt).reshape(1, 1, 4)
        C = (fr.astype(np.float64) / 255).astype(np.float32) if dt == np.uint8 else fr.astype(np.float32)
        for radius in (1, 2):
            for gamma in (0.0, 1.0, 2.5):
                lo, hi = color_bounds(fr, radius, gamma)
                assert np.array_equal(lo[0, 0, :3], C[0, 0, :3].astype(np.float64)) and np.array_equal(hi, lo) and lo[0, 0, 3] == 1


def test_a_constant_frame_is_its_own_box_and_counts_its_windows():
    c = np.float32([0.1, 1 / 3, 1e4, 0.5])
    fr = np.broadcast_to(c, (7, 9, 4)).copy()
    for radius in (1, 2):
        lo, hi = color_bounds(fr, radius, 2.5)
        assert np.array_equal(lo[..., :3], np.broadcast_to(c[:3].astype(np.float64), (7, 9, 3))) and np.array_equal(lo, hi)
        k = 2 * radius + 1
        ny = np.minimum(np.arange(7) + radius, 6) - np.maximum(np.arange(7) - radius, 0) + 1
        nx = np.minimum(np.arange(9) + radius, 8) - np.maximum(np.arange(9) - radius, 0) + 1
        assert np.array_equal(lo[..., 3], np.outer(ny, nx)) and lo[..., 3].max() == k * k and lo[0, 0, 3] == (radius + 1) ** 2


def test_a_window_that_is_all_nan_is_the_whole_line():
    fr = np.full((5, 5, 4), 0.5, np.float32)
    fr[:3, :3, 1] = np.nan                           # one NaN channel makes the texel not valid
    fr[0, 4, 0] = np.inf
    lo, hi = color_bounds(fr, 1, 1.0)
    assert (lo[:2, :2, :3] == -np.inf).all() and (hi[:2, :2, :3] == np.inf).all() and not lo[:2, :2, 3].any()
    assert lo[2, 2, 3] == 5 and np.array_equal(lo[2, 2, :3], [0.5, 0.5, 0.5]) and np.array_equal(hi[2, 2], lo[2, 2])
    assert lo[0, 3, 3] == 3 and lo[1, 4, 3] == 5     # (0, 3): (0, 3), (1, 3), (1, 4) -- not the NaN column 2 nor the Inf texel (0, 4)
    lo2, _ = color_bounds(fr, 2, 1.0)
    assert lo2[0, 0, 3] == 0 and lo2[1, 1, 3] == 3 + 4     # rows 0..2: column 3 only; row 3: columns 0..3


def test_corner_windows_by_hand():
    """4 x 4 of the values 0..15 in R, twice that in G, a constant B.  The corner pixel's 3 x 3 window holds n = 4 texels
    {0, 1, 4, 5}: mean 2.5, variance (2.5^2 + 1.5^2 + 1.5^2 + 2.5^2) / 4 = 4.25; its 5 x 5 window holds n = 9 texels {0, 1, 2, 4, 5, 6, 8, 9, 10}:
    mean 5, variance (25 + 16 + 9 + 1 + 0 + 1 + 9 + 16 + 25) / 9 = 34 / 3."""
    v = np.arange(16, dtype=np.float32).reshape(4, 4)
    fr = np.stack([v, 2 * v, np.full((4, 4), 3, np.float32), np.ones((4, 4), np.float32)], -1)
    lo, hi = color_bounds(fr, 1, 2.0)
    s = np.sqrt(4.25)
    assert lo[0, 0, 3] == 4 and np.allclose(lo[0, 0, :3], [2.5 - 2 * s, 5 - 4 * s, 3], rtol=1e-15) and np.allclose(hi[0, 0, :3], [2.5 + 2 * s, 5 + 4 * s, 3], rtol=1e-15)
    lo, hi = color_bounds(fr, 2, 0.5)
    s = np.sqrt(34 / 3)
    assert lo[0, 0, 3] == 9 and np.allclose(lo[0, 0, :3], [5 - 0.5 * s, 10 - s, 3], rtol=1e-15) and np.allclose(hi[0, 0, :3], [5 + 0.5 * s, 10 + s, 3], rtol=1e-15)
    assert lo[1, 1, 3] == 16 and lo[3, 3, 3] == 9


def test_the_mean_is_rounded_to_float32_before_the_deviations():
    fr = np.zeros((1, 3, 4), np.float32)
    fr[0, :, 0] = [1.0, 1.0, 1.0 + 2.0 ** -23]      # the mean 1 + 2^-23 / 3 rounds to 1
    lo, hi = color_bounds(fr, 1, 1.0)
    sigma = np.sqrt((2.0 ** -23) ** 2 / 3)
    assert lo[0, 1, 0] == 1.0 - sigma and hi[0, 1, 0] == 1.0 + sigma
