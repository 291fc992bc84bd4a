"""The input recipe of the median filters' GPU tests (tests/test_gpu_median*.py), held to its conditions by the float64 checker alone
in tests/test_median_args.py -- no kernel takes part in choosing it.

A frame is noisy `albedo x smooth light` (gamma noise) with 5 % of its pixels replaced by 0 or 50.  Guide layer 0 is the clean albedo
as uint8 codes: blocky, the block levels multiples of 51 codes (0.2), plus a small ramp (3 x + 5 y) % 7 codes that is not symmetric
about any pixel, so that two taps of a window seldom weigh the same and the weighted sums seldom tie.  SIGMA0 = 0.02: a tap across a
block edge has arg <= -72 (it does not matter: 2^-72 against the centre's 1), a tap inside the block arg >= -3.1.  Further layers are
ramps alone, (a_l x + b_l y) % 5 codes at SIGMA_REST = 0.1, 0.06 of arg each at most: with 16 layers the largest |arg| that matters is
A <= 4.1, inside the header's condition (3 L' + 2) A <= 295 (50 x 4.1 = 205).
"""
import numpy as np

SIGMA0, SIGMA_REST = 0.02, 0.1
RADII = (1, 2, 3)
LAYER_COUNTS = (0, 1, 3, 4, 5, 16)
TILE_W, TILE_H, GLOBAL_H = 64, 16, 4        # the geometry built (csrc/median_tile.hpp; the global class: 64 x 4 pixels per workgroup)
NEAR_SHARE = 0.02                           # pixel-channels with margin <= delta: at most this share, in every case the GPU tests use


def scene(h, w, seed=0, gain=1.0, block=6):
    """(noisy, guide0, clean): float32 (h, w, 4), uint8 (h, w, 4), float32 (h, w, 4); alpha of the frame is a ramp."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    B = block
    levels = rng.integers(1, 5, (h // B + 1, w // B + 1, 3)).repeat(B, 0).repeat(B, 1)[:h, :w] * 51
    codes = levels + ((3 * xx + 5 * yy) % 7)[..., None]
    alb = codes / 255.0
    light = np.stack([0.6 + 0.3 * np.sin(xx * 0.05), 0.6 + 0.3 * np.cos(yy * 0.06), 0.5 + 0.2 * np.sin((xx + yy) * 0.04)], -1)
    clean = alb * light * gain
    noisy = clean * rng.gamma(16.0, 1 / 16.0, (h, w, 3))
    hit = rng.random((h, w)) < 0.05
    noisy[hit] = np.where(rng.random((int(hit.sum()), 1)) < 0.5, 0.0, 50.0 * gain)
    alpha = ((xx + 2 * yy) % 17 / 16.0)[..., None]
    guide0 = np.concatenate([codes, np.full((h, w, 1), 255)], -1).astype(np.uint8)
    return (np.concatenate([noisy, alpha], -1).astype(np.float32), guide0, np.concatenate([clean, alpha], -1).astype(np.float32))


def layer_set(guide0, n_layers, dtype=np.uint8):
    """(layers, sigmas) of n_layers layers in `dtype`: guide0 first, then ramps.  A float layer holds code / 255 in that dtype (float16
    rounds; the checker reads what the kernel reads)."""
    h, w = guide0.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    layers = [guide0]
    for l in range(1, n_layers):
        ramp = ((l + 1) * xx + (2 * l + 3) * yy) % 5
        layers.append(np.stack([ramp, (ramp + l) % 5, (2 * ramp + 1) % 5, np.full((h, w), 255)], -1).astype(np.uint8))
    layers = layers[:n_layers]
    dtype = np.dtype(dtype)
    if dtype != np.uint8:
        layers = [(lyr.astype(np.float32) / np.float32(255)).astype(dtype) for lyr in layers]
    return layers, [SIGMA0] + [SIGMA_REST] * (n_layers - 1) if n_layers else []


def as_dtype(img, dtype):
    """A float32 image in a frame dtype: uint8 by rounding 255 x (clipped), float16 by rounding (50 is a half; 50 x 1024 is not: Inf)."""
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.clip(np.rint(img * 255.0), 0, 255).astype(np.uint8)
    with np.errstate(over="ignore"):
        return img.astype(dtype)


def seam_shapes(n_layers):
    """(h, w) from 1 x 1, through frames smaller than the window, to one past the wave and tile seams: widths 63, 64, 65 and 129,
    heights one past the tile height of the class that n_layers runs in."""
    th = TILE_H if n_layers <= 4 else GLOBAL_H
    return [(1, 1), (1, 2), (2, 1), (2, 3), (3, 3), (5, 6), (3, 63), (th, 64), (th + 1, 65), (2 * th + 1, 129), (th + 1, 5)]


def exact_scene(h, w, seed=0):
    """(frame, guide): a float32 frame of small integers / 8 with fireflies and NaN / Inf texels, and a float32 guide of INTEGER levels
    0 .. 3 in blocks of 5.  With EXACT_SIGMA a tap of another level has arg <= -7213 (weight exactly 0) and a tap of the same level
    arg = 0 (weight exactly 1): every sum is an integer."""
    rng = np.random.default_rng(seed)
    frame = (rng.integers(0, 64, (h, w, 4)) / 8.0).astype(np.float32)
    spots = rng.random((h, w, 3)) < 0.03
    frame[..., :3][spots] = rng.choice(np.float32([np.nan, np.inf, -np.inf, 4096.0, -3.0]), int(spots.sum()))
    lev = rng.integers(0, 4, (h // 5 + 1, w // 5 + 1, 1)).repeat(5, 0).repeat(5, 1)[:h, :w]
    guide = np.concatenate([lev, 3 - lev, lev % 2, np.ones_like(lev)], -1).astype(np.float32)
    return frame, guide


def planted(h, w, where, seed=0):
    """(frame, float32 guide) of the recipe with NaN / +-Inf planted on corners, edges and every seam of the 64 x 16 and 64 x 4 grids, in the
    frame ("in"), in the guide ("guide") or in both; and a non-finite alpha in each, which does not count."""
    noisy, g0, _ = scene(h, w, seed=seed)
    guide = (g0.astype(np.float32) / np.float32(255))
    xs = sorted({x for x in (0, w - 1, w // 2, 63, 64, 65, 127, 128) if 0 <= x < w})
    ys = sorted({y for y in (0, h - 1, h // 2, 3, 4, 15, 16, 17, 31, 32) if 0 <= y < h})
    for k, (y, x) in enumerate([(y, x) for y in ys for x in xs]):
        bad = (np.nan, np.inf, -np.inf)[k % 3]
        if where in ("in", "both"):
            noisy[y, x, k % 3] = bad
        if where in ("guide", "both"):
            guide[y, x, (k + 1) % 3] = bad
    noisy[h // 3, w // 3, 3] = np.nan
    guide[h // 3, w // 4, 3] = np.inf
    return noisy, guide


def strip(h, w):
    """(frame, uint8 guide) of a strip one pixel wide or high: the recipe's shape in one dimension, blocks of 48, 5 % of the pixels 50, one NaN."""
    n = h * w
    rng = np.random.default_rng(h + w)
    codes = rng.integers(1, 5, (n // 48 + 1, 3)).repeat(48, 0)[:n] * 51 + (np.arange(n) * 3 % 7)[:, None]
    guide = np.concatenate([codes, np.full((n, 1), 255)], -1).astype(np.uint8).reshape(h, w, 4)
    frame = np.ones((n, 4), np.float32)
    frame[:, :3] = codes / 255.0 * rng.gamma(16.0, 1 / 16.0, (n, 3))
    frame[rng.random(n) < 0.05, :3] = 50.0
    frame[n // 3, 0] = np.nan
    return frame.reshape(h, w, 4), guide


HUGE_PATTERN, HUGE_SIGMA = (37, 41), 0.5


def huge_patterns():
    """(frame pattern, guide pattern): the two uint8 37 x 41 patterns the 16400 x 16400 frame and guide are tiled from."""
    rng = np.random.default_rng(84)
    return rng.integers(0, 256, HUGE_PATTERN + (4,), dtype=np.uint8), rng.integers(0, 256, HUGE_PATTERN + (4,), dtype=np.uint8)


EXACT_SIGMA = 0.01


# What the filter is for (tests/test_gpu_median_demo.py; the float64 side is tests/test_median_args.py): the recipe's frame at 40 x 70,
# radius 2, layer 0 alone at DEMO_SIGMA.  The three mse ratios were measured in float64 with tests/np_median.py and
# tests/np_bilateral_joint.py and are written here with a factor-2 margin towards "easier".
DEMO_SHAPE, DEMO_RADIUS, DEMO_SIGMA = (40, 70), 2, 0.02
DEMO_PLAIN_RATIO = 1.7e-4       # mse(plain median) <= DEMO_PLAIN_RATIO * mse(input)                     (float64: 0.0050 / 61.6 = 8.1e-5)
DEMO_WEIGHTED_RATIO = 0.6       # mse(weighted median) <= DEMO_WEIGHTED_RATIO * mse(plain median)        (float64: 0.00147 / 0.0050 = 0.29)
DEMO_BILATERAL_RATIO = 2000     # mse(joint bilateral) >= DEMO_BILATERAL_RATIO * mse(weighted median)    (float64: 6.09 / 0.00147 = 4141)


def demo():
    """(noisy, guide0, clean) of the demonstration."""
    return scene(*DEMO_SHAPE, seed=7)


def mse(a, b):
    return float(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2))
