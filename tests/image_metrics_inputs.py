"""The recipe of the image-metrics GPU tests (tests/test_gpu_image_metrics*.py), held to its conditions on the CPU by
tests/test_image_metrics_args.py with the checker alone.

    b = smooth shading times a texture;  a = b + noise whose amplitude ramps across the frame, from nothing at the left edge (ssim near 1)
    to several times the texture's contrast at the right edge (ssim near 0, and S_ab < 0 where the noise happens to oppose the texture).

pair(h, w, scale): float32 (a, b) with radiance times `scale` (compare with peak = scale).  as_dtype: a frame in one of the three
formats (uint8 through the rounding of a u8 encoder, float16 by rounding to nearest even)."""
import numpy as np

SHAPES = [(1, 1), (7, 1), (5, 5), (11, 11), (15, 63), (16, 64), (17, 65), (33, 129)]      # (h, w): 1 x 1, 1 x 7, ... 129 x 33 in w x h
DTYPES = [np.uint8, np.float16, np.float32]


def pair(h, w, scale=1.0, seed=7):
    rng = np.random.default_rng(seed + 1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    shade = 0.45 + 0.25 * np.sin(xx * 0.045 + 0.4) * np.cos(yy * 0.11)
    texture = 1.0 + 0.35 * np.sin(xx * 1.1) * np.sin(yy * 0.9 + 0.5)
    tint = np.array([1.0, 0.85, 0.7])
    b = shade[..., None] * texture[..., None] * tint
    ramp = (xx / max(w - 1, 1)) ** 2                                      # 0 at the left edge, 1 at the right
    a = b + 0.45 * ramp[..., None] * rng.standard_normal((h, w, 1)) * tint + 0.02 * ramp[..., None] * rng.standard_normal((h, w, 3))
    a, b = np.clip(a, 0.0, 1.0), np.clip(b, 0.0, 1.0)
    one = np.ones((h, w, 1))
    return (np.concatenate([a, one], -1) * scale).astype(np.float32), (np.concatenate([b, one], -1) * scale).astype(np.float32)


def as_dtype(x, dtype):
    """A float32 unit-range frame in `dtype`."""
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return np.clip(np.rint(x * 255.0), 0, 255).astype(np.uint8)
    return x.astype(dtype)
