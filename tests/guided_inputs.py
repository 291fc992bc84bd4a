"""The input recipe of the guided filter's GPU tests (tests/test_gpu_guided*.py), held to its conditions by the float64 checker alone
in tests/test_guided_args.py -- no kernel takes part in choosing it.

A frame is noisy `albedo x smooth light`; the guide is the clean albedo, blocky with blocks of 4 radii, so that a quarter of the
windows see a constant guide (the filter averages) and the windows across a block edge see a large covariance (the regression
carries the edge).  EPS = 1e-3.  With a unit-range guide D <= 0.8 and every texel valid n_min = (radius + 1)^2 >= 4, so
D^2 / eps <= 640 <= 2^10 n_min: the condition of the header's precision clause.
"""
import numpy as np

EPS = 1e-3
RADII = (1, 2, 3, 8, 16)
# the geometry built (csrc/guided_box.hpp): 256 lanes, strips of 256 - 2 r columns, segments of 32 rows, waves of 64 lanes
LANES, PERIOD, WAVE = 256, 32, 64


def strip_w(radius):
    return LANES - 2 * radius


def scene(h, w, radius, seed=0, gain=1.0):
    """(noisy, albedo, clean): float32 (h, w, 4) each; alpha of the frame is a ramp (so that out.a == in.a says something)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    B = 4 * radius
    alb = (0.15 + 0.8 * rng.random((h // B + 1, w // B + 1, 3))).repeat(B, 0).repeat(B, 1)[:h, :w]
    light = np.stack([0.6 + 0.3 * np.sin(xx * 0.05), 0.6 + 0.3 * np.cos(yy * 0.06), 0.5 + 0.2 * np.sin((xx + yy) * 0.04)], -1)
    clean = alb * light * gain
    noisy = clean * rng.gamma(4.0, 1 / 4.0, (h, w, 3))
    alpha = ((xx + 2 * yy) % 17 / 16.0)[..., None]
    one = np.ones((h, w, 1))
    return (np.concatenate([noisy, alpha], -1).astype(np.float32), np.concatenate([alb, one], -1).astype(np.float32),
            np.concatenate([clean, alpha], -1).astype(np.float32))


def as_dtype(img, dtype):
    """A float32 image in a frame dtype: uint8 by rounding 255 x (clipped), float16 by rounding."""
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.clip(np.rint(img * 255.0), 0, 255).astype(np.uint8)
    return img.astype(dtype)


def depth_guide(h, w, radius, seed=0):
    """A depth-like guide in its own units: planes about 300 units away, stepping by tens of units at block edges, the three
    channels three different mixes.  Used with eps = DEPTH_EPS: D <= 30 gives D^2 / eps <= 900."""
    rng = np.random.default_rng(seed + 100)
    B = 4 * radius
    z = (300.0 + 25.0 * rng.random((h // B + 1, w // B + 1, 3))).repeat(B, 0).repeat(B, 1)[:h, :w]
    return np.concatenate([z, np.ones((h, w, 1))], -1).astype(np.float32)


DEPTH_EPS = 1.0


def seam_shapes(radius):
    """(h, w) from 1 x 1, through frames smaller than the window, to one past every seam of the geometry: wave, strip, restart."""
    sw = strip_w(radius)
    return [(1, 1), (1, 2), (2, 1), (radius, radius + 1), (2 * radius + 1, 2 * radius), (3, WAVE + 1), (PERIOD + 1, 5),
            (5, sw), (7, sw + 1), (PERIOD + 1, sw + 1), (2 * PERIOD + 1, 9), (3, LANES + 1), (9, 2 * sw + 1)]


# What the filter is for (tests/test_gpu_guided_demo.py; the float64 side is tests/test_guided_args.py): a 70 x 130 frame of noisy
# `albedo x smooth light` with the clean, blocky albedo (blocks of 5) as the guide, radius 8.
DEMO_RADIUS, DEMO_EPS = 8, 1e-3
DEMO_GUIDED_RATIO = 1 / 20      # mse(guided) <= mse(input) / 20           -- asserted of the checker, then of the kernel
DEMO_SELF_RATIO = 10            # mse(self-guided) >= 10 mse(guided)


def demo():
    """(noisy, albedo, clean): float32 (70, 130, 4)."""
    h, w = 70, 130
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    alb = (0.15 + 0.8 * rng.random((h // 5 + 1, w // 5 + 1, 3))).repeat(5, 0).repeat(5, 1)[:h, :w]
    light = np.stack([0.6 + 0.3 * np.sin(xx * 0.05), 0.6 + 0.3 * np.cos(yy * 0.06), 0.5 + 0.2 * np.sin((xx + yy) * 0.04)], -1)
    clean = alb * light
    noisy = clean * rng.gamma(4.0, 1 / 4.0, (h, w, 3))
    one = np.ones((h, w, 1))
    return tuple(np.concatenate([x, one], -1).astype(np.float32) for x in (noisy, alb, clean))
