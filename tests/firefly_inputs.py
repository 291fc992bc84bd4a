"""The input recipe of the firefly tests (section a4l), shared by tests/test_firefly_args.py, which holds the recipe to its
conditions with the checker alone, and the GPU tests, which feed the same frames to the kernel.

    float frames: log-uniform radiance 1e-2 .. 1e1 per channel, alpha uniform in [0, 1); one texel in fifty has its RGB times 4096;
                  one NaN, one +Inf, one -Inf and one -2.0 channel planted (frames of 64 pixels and more);
    uint8 frames: uniform random codes.
"""
import numpy as np

SHAPES = ((67, 131), (17, 65), (16, 64))             # (h, w) the recipe is held to its conditions on
PARAMS = tuple((radius, rank) for radius in (1, 2) for rank in (1, 2, 3, 4))
GAIN_FLOOR = ((1.0, 0.0), (1.5, 0.25))
PLANTED = (np.nan, np.inf, -np.inf, -2.0)


def frame_of(shape, dt, seed=0):
    h, w = shape
    rng = np.random.default_rng([300, seed])
    if np.dtype(dt) == np.uint8:
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    f = np.exp(rng.uniform(np.log(1e-2), np.log(1e1), (h, w, 4)))
    f[..., 3] = rng.random((h, w))
    f[..., :3] *= np.where(rng.random((h, w, 1)) < 1 / 50, 4096.0, 1.0)
    with np.errstate(over="ignore"):
        f = f.astype(dt)                             # (float16: 4096 x radiance above 16 overflows to +Inf, one more texel to repair)
    flat = f.reshape(-1, 4)
    if len(flat) >= 64:
        for i, v in enumerate(PLANTED):              # one channel each, texels apart from each other
            flat[7 + 13 * i, i % 3] = v
    return f


def plant(frame, ys, xs, values=(4096.0, np.nan, np.inf, -np.inf)):
    """A copy of a float frame with fireflies (RGB times 4096), NaN and +-Inf channels planted in turn on the pixels ys x xs."""
    f = frame.copy()
    h, w = f.shape[:2]
    n = 0
    for y in ys:
        for x in xs:
            if not (0 <= y < h and 0 <= x < w):
                continue
            v = values[n % len(values)]
            if np.isfinite(v):
                with np.errstate(over="ignore"):
                    f[y, x, :3] = (f[y, x, :3].astype(np.float32) * np.float32(v)).astype(f.dtype)
            else:
                f[y, x, n % 3] = v
            n += 1
    return f
