"""The input recipe of the history-clip tests (include/mi_denoise.h, section a4m), shared by tests/test_history_clip_args.py, which
holds the recipe to its conditions with the checkers alone, and the GPU tests, which feed the same arrays to the kernels.

    frames   a radiance that varies over hundreds of texels (a reprojection by a few texels does not leave the box) times per-texel
             gamma noise of relative deviation 0.3; uint8 frames are its [0, 1] part.
    history  the colour is the frame's noise-free radiance times a factor that is constant over blocks of 12 x 12 texels: 1 in half
             of the blocks (the history lies inside the box of most pixels, whatever gamma in 0.5 .. 2), 3 or 0.1 in the others (it lies
             outside in at least one channel).  The state is tests/temporal_accumulate_inputs.py's.
    layers, sigmas, motion, settings: tests/temporal_accumulate_inputs.py's, so a part of the history is rejected (S == 0), a part
             believed and a part half believed; the motions are "none", "integer" and "fractional".
    clip planes: np_color_bounds.color_bounds of the frame, rounded to float32 (the GPU tests take the kernel's own).

The conditions, on 261 x 131, for every motion, every L in LAYERS, both radii and gamma in {0.5, 2}: among the pixels with S > 0 at
least a fifth have a channel clipped and at least a fifth have none clipped.

Measured with the checkers (test_history_clip_args.py prints them): the share of the pixels with S > 0 that have a channel clipped,
its smallest and largest value over the three motions and L = 0, 1, 3, 16 (S > 0 on 0.74 .. 1.00 of the pixels):
                         float32 frames    uint8 frames
    gamma 0.5, radius 1   0.715 .. 0.735    0.718 .. 0.737
    gamma 0.5, radius 2   0.478 .. 0.517    0.487 .. 0.525
    gamma 2,   radius 1   0.437 .. 0.469    0.438 .. 0.472
    gamma 2,   radius 2   0.435 .. 0.461    0.435 .. 0.465
so both shares lie between 0.26 and 0.74 everywhere.
"""
import numpy as np

import temporal_accumulate_inputs as tai
from np_color_bounds import color_bounds

SHAPE = (131, 261)                                   # (h, w) the recipe is held to its conditions on
MOTIONS = ("none", "integer", "fractional")
LAYERS = (0, 1, 3, 16)
GAMMAS = (0.5, 2.0)
SETTINGS = tai.SETTINGS
layers_of, sigmas_of, motion_of, var_spatial_of = tai.layers_of, tai.sigmas_of, tai.motion_of, tai.var_spatial_of


def radiance(shape, t=1, scale=1.0):
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return scale * np.stack([0.55 + 0.25 * np.sin(xx * 0.012 + 0.2 * t), 0.5 + 0.2 * np.cos(yy * 0.015), 0.45 + 0.2 * np.sin((xx + yy) * 0.008)], -1)


def frame_of(shape, t=1, dtype=np.float32, scale=1.0):
    h, w = shape
    rng = np.random.default_rng(17000 + t)
    rgb = radiance(shape, t, scale) * rng.gamma(11.0, 1 / 11.0, (h, w, 3))          # relative deviation 0.30
    img = np.concatenate([rgb, rng.random((h, w, 1))], -1)
    if np.dtype(dtype) == np.uint8:
        return (np.clip(img, 0, 1) * 255).astype(np.uint8)
    return img.astype(dtype)


def history_of(shape, t=1, scale=1.0, seed=0):
    """(colour, state): float32 (h, w, 4) each."""
    h, w = shape
    rng = np.random.default_rng(19000 + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    factor = rng.choice([1.0, 1.0, 3.0, 0.1], (h // 12 + 1, w // 12 + 1))[yy // 12, xx // 12]
    col = np.concatenate([radiance(shape, t, scale) * factor[..., None], rng.random((h, w, 1))], -1).astype(np.float32)
    return col, tai.history_of(shape, seed)[1]


def boxes_of(frame, radius, gamma):
    """The checker's box as the float32 planes a call is given."""
    with np.errstate(over="ignore"):
        lo, hi = color_bounds(frame, radius, gamma)
    return lo.astype(np.float32), hi.astype(np.float32)


def case(shape, L, fdt, gdt, motion, with_var, setting, t=1, hist="recipe", scale=1.0):
    """((frame, layers, prev_layers, sigmas), keywords) of one accumulation, without the clip planes."""
    kw = dict(hist=history_of(shape, t, scale) if isinstance(hist, str) else hist, motion=motion_of(shape, motion),
              var_spatial=var_spatial_of(shape) if with_var else None, **SETTINGS[setting])
    return (frame_of(shape, t, fdt, scale), layers_of(shape, L, gdt, t), layers_of(shape, L, gdt, t - 1), sigmas_of(L)), kw


# ---- the demonstration of tests/test_gpu_sequence_atrous_recursive_clip.py -----------------------------------------------------
DEMO_SHAPE, DEMO_A, DEMO_B, DEMO_SWITCH, DEMO_FRAMES = (67, 131), 0.75, 0.25, 6, 8
DEMO_SQUARE = (slice(16, 48), slice(48, 80))         # 32 x 32, its centre (32, 64)
DEMO_CENTRE = (32, 64)


def demo_frames():
    """Noise-free grey frames of B with a 32 x 32 square of A; from frame DEMO_SWITCH on the square is B too.  One constant layer."""
    frames = []
    for t in range(DEMO_FRAMES):
        f = np.full(DEMO_SHAPE + (4,), DEMO_B, np.float32)
        f[..., 3] = 1.0
        if t < DEMO_SWITCH:
            f[DEMO_SQUARE + (slice(0, 3),)] = DEMO_A
        frames.append(f)
    layers = [[np.full(DEMO_SHAPE + (4,), 128, np.uint8)] for _ in range(DEMO_FRAMES)]
    return frames, layers
