"""Inputs of the temporal-accumulation tests (include/mi_denoise.h, section a4j), shared by the CPU and the GPU suites.

    * frames: a smooth HDR-range radiance times per-frame noise; uint8 frames are its clipped [0, 1] part.
    * layers: layer 0 is a LABEL plane -- blocks of 24 x 24 texels with one of four ids, which move by (3, 2) texels per frame,
      whatever the motion field says -- with a sigma so small that a different id weighs exactly 0 (in fp32 and in float64: the
      exponent is below -1000).  Layers 1.. are static ramps plus per-frame noise whose amplitude grows from left to right, in
      units of the layer's sigma and divided by sqrt(L - 1): the product of their weights runs from about 0.99 at the left edge to
      about 0.07 at the right one, for every L.  So with three layers and more a history is believed in full, in part and not at
      all in different parts of one image (tests/test_temporal_accumulate_args.py holds the input to that).
    * motion: None, a constant integer vector, a constant fractional one, and a smooth field of up to +-6 texels that points off the
      frame along parts of every edge.
    * histories: a colour plane, and a state (m1, m2, N, 0) with N in [1, 40).
"""
import numpy as np

MOTIONS = ("none", "integer", "fractional", "smooth")
SETTINGS = (dict(alpha=0.2, alpha_moments=0.2, history_max=32, history_full=4),
            dict(alpha=0.05, alpha_moments=0.5, history_max=8, history_full=2.5))


def frame_of(shape, t, dtype=np.float32):
    h, w = shape
    rng = np.random.default_rng(7000 + t)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([0.6 + 0.4 * np.sin(xx * 0.11 + 0.3 * t), 0.5 + 0.5 * np.cos(yy * 0.07), 0.4 + 0.3 * np.sin((xx + yy) * 0.05), np.ones_like(xx)], -1)
    img = base * np.concatenate([rng.gamma(8.0, 1 / 8.0, (h, w, 3)), np.ones((h, w, 1))], -1) * (1.0 if np.dtype(dtype) == np.uint8 else 1.6)
    if np.dtype(dtype) == np.uint8:
        return (np.clip(img, 0, 1) * 255).astype(np.uint8)
    return img.astype(dtype)


def labels_of(shape, t):
    """Ids 0..3 in blocks of 24 x 24 that move by (3, 2) texels per frame."""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx - 3 * t) // 24) + 2 * ((yy - 2 * t) // 24)) % 4


def sigmas_of(L):
    return ([0.01] + [0.1 + 0.01 * l for l in range(1, L)])[:L]


def layers_of(shape, L, dtype, t):
    """L guide layers of frame t; uint8 values c stand for c / 255, float layers hold c / 255."""
    h, w = shape
    rng = np.random.default_rng(9000 + t)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    sg = sigmas_of(L)
    out = []
    for l in range(L):
        if l == 0:
            lab = labels_of(shape, t).astype(np.float64)
            v = np.stack([lab * 85, (3 - lab) * 85, np.full((h, w), 128.0), np.full((h, w), 255.0)], -1)
        else:
            amp = (0.05 + 0.9 * xx / max(w, 1)) / np.sqrt(L - 1)
            ramp = np.stack([40 + (xx * 0.5 + 7 * l) % 150, 40 + (yy * 0.7 + 11 * l) % 150, 40 + ((xx + yy) * 0.3 + 13 * l) % 150, np.full((h, w), 255.0)], -1)
            v = ramp + np.concatenate([rng.normal(0, 1, (h, w, 3)) * (amp * sg[l] * 255)[..., None], np.zeros((h, w, 1))], -1)
        v = np.clip(np.round(v), 0, 255)
        out.append(v.astype(np.uint8) if np.dtype(dtype) == np.uint8 else (v / 255).astype(dtype))
    return out


def motion_of(shape, kind):
    h, w = shape
    if kind == "none":
        return None
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "integer":
        m = np.stack([np.full((h, w), 3.0), np.full((h, w), -2.0)], -1)
    elif kind == "fractional":
        m = np.stack([np.full((h, w), 2.5), np.full((h, w), -1.25)], -1)
    else:
        m = np.stack([6 * np.sin(xx * 0.05 + 0.4) * np.cos(yy * 0.07), 6 * np.cos(xx * 0.03 + yy * 0.05 + 1.0)], -1)
    return m.astype(np.float32)


def history_of(shape, seed=0):
    """(colour, state): float32 (h, w, 4) each; state = (m1, m2 >= m1^2, N in [1, 40), 0)."""
    h, w = shape
    rng = np.random.default_rng(11000 + seed)
    col = np.concatenate([rng.gamma(4.0, 0.25, (h, w, 3)), np.ones((h, w, 1))], -1).astype(np.float32)
    m1 = rng.uniform(0.1, 1.5, (h, w))
    st = np.stack([m1, m1 * m1 + rng.uniform(0, 0.2, (h, w)), rng.uniform(1, 40, (h, w)), np.zeros((h, w))], -1).astype(np.float32)
    return col, st


def var_spatial_of(shape, seed=0):
    return np.random.default_rng(13000 + seed).uniform(0, 0.3, shape).astype(np.float32)
