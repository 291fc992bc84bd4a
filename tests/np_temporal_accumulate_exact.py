"""Exact answers of the recursive temporal accumulation (include/mi_denoise.h, section a4j), after np_atrous_exact.py's construction.

    * frames and history colours are GREY integers in multiples of 16 (alpha an integer multiple of 16 too), the history moments
      m1, m2 integers in multiples of 16, the history lengths 1, 3 or 7;
    * the guide layers are label planes of two values at sigma 0.02: 2^arg is exactly 1 (every label equal) or exactly 0;
    * motion comes in integers and halves: bw is 0, 1/4, 1/2 or 1.

Then every w is 0, 1/4, 1/2 or 1 and the sums S, hc, h1, h2, hn are multiples of 1/4 far below 2^24: exact in fp32 in ANY order of
the taps, so the answer does not depend on how a kernel schedules them -- but it does depend on which texel every weight meets, on
which taps are skipped, and on N' being the UNNORMALISED sum.  Everything after the sums is a fixed sequence of single fp32
operations (divisions, 1 / N', subtractions, FMAs), which this file evaluates bit-true: products and differences of fp32 values
are exact in float64, a quotient rounds correctly through float64 (53 >= 2 * 24 + 2), and an FMA is rounded once with the help of
the exact error of the float64 sum.  With alpha below 1/8 and equal history lengths 1 / N' is a power of two, 1/2, 1/4 or 1/8.
"""
import numpy as np

SIGMA = 0.02
F32 = np.float32
LR, LG, LB = F32(0.2126), F32(0.7152), F32(0.0722)


def fma32(a, b, c):
    """round32(a b + c) for float32 arrays, one rounding: the product is exact in float64; the float64 sum is corrected by its exact
    error (TwoSum) where it sits on a float32 tie that the exact sum does not sit on."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    tie = (s.view(np.int64) & 0x1fffffff) == 0x10000000             # the 29 bits below a float32 mantissa: exactly one half
    s = np.where(tie & (err != 0), np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)      # towards the exact sum
    return s.astype(np.float32)


def lum32(C):
    C = np.asarray(C, np.float32)
    t = (LR.astype(np.float64) * C[..., 0].astype(np.float64)).astype(np.float32)
    return fma32(LB, C[..., 2], fma32(LG, C[..., 1], t))


def label_layers(shape, L, t, seed=5):
    """L label planes of frame t (uint8, values 40 and 200): random blocks of 8 x 8 texels; those of layers 0 and 1 move by (2, 1)
    texels per frame, those of layer 2 stand still, and the layers past the third are constant planes (rejection enough already)."""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for l in range(L):
        blocks = np.random.default_rng([seed, l]).integers(0, 2, (h // 8 + 4, w // 8 + 4))
        if l >= 3:
            blocks[:] = l % 2
        dy, dx = (t, 2 * t) if l < 2 else (0, 0)
        v = np.where(blocks[((yy - dy) // 8) % blocks.shape[0], ((xx - dx) // 8) % blocks.shape[1]] == 1, 200, 40)
        out.append(np.stack([v, 255 - v, v, np.full((h, w), 255)], -1).astype(np.uint8))
    return out


def grey_frame(shape, seed):
    h, w = shape
    rng = np.random.default_rng([seed, 1])
    g = 16.0 * rng.integers(0, 16, (h, w))
    return np.stack([g, g, g, 16.0 * rng.integers(0, 16, (h, w))], -1).astype(np.float32)


def history(shape, seed):
    h, w = shape
    rng = np.random.default_rng([seed, 2])
    col = grey_frame(shape, seed + 50)
    st = np.stack([16.0 * rng.integers(0, 16, (h, w)), 16.0 * rng.integers(0, 64, (h, w)), rng.choice([1.0, 3.0, 7.0], (h, w)), np.zeros((h, w))], -1)
    return col, st.astype(np.float32)


def motion(shape, seed):
    """Integers and halves in [-3, 3], constant over blocks of 5 x 3 texels."""
    h, w = shape
    rng = np.random.default_rng([seed, 3])
    m = rng.integers(-6, 7, (h // 3 + 1, w // 5 + 1, 2)) / 2.0
    yy, xx = np.mgrid[0:h, 0:w]
    return m[yy // 3, xx // 5].astype(np.float32)


def temporal_accumulate_exact(frame, layers, prev_layers, hist, mv, alpha, alpha_moments, history_max):
    """(colour, state, Vt) as float32, bit for bit what section a4j prescribes, and the fraction of taps the layers rejected."""
    C = np.asarray(frame, np.float32)
    Hc, Hs = (np.asarray(a, np.float32).astype(np.float64) for a in hist)
    h, w = C.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    pp = np.stack([xx, yy], -1) + np.asarray(mv, np.float64)          # integers and halves: exact in fp32 and here
    assert np.array_equal(pp * 2, np.round(pp * 2))
    ok = (pp[..., 0] > -1) & (pp[..., 0] < w) & (pp[..., 1] > -1) & (pp[..., 1] < h)
    x0, y0 = np.floor(pp[..., 0]).astype(np.int64), np.floor(pp[..., 1]).astype(np.int64)
    fx, fy = pp[..., 0] - x0, pp[..., 1] - y0
    S, hc, hs = np.zeros((h, w)), np.zeros((h, w, 4)), np.zeros((h, w, 3))
    offered = rejected = 0
    for b in (0, 1):
        for a in (0, 1):
            bw = (fx if a else 1 - fx) * (fy if b else 1 - fy)
            qx, qy = x0 + a, y0 + b
            take = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & (bw != 0)
            py, px = np.nonzero(take)
            ty, tx = qy[take], qx[take]
            same = np.ones(py.size, bool)
            for gc, gp in zip(layers, prev_layers):
                same &= (gc[py, px, :3] == gp[ty, tx, :3]).all(-1)
            offered += py.size
            rejected += int((~same).sum())
            wt = bw[take] * same
            S[py, px] += wt
            hc[py, px] += wt[:, None] * Hc[ty, tx]
            hs[py, px] += wt[:, None] * Hs[ty, tx, :3]
    for v in (S, hc, hs):
        assert np.array_equal(v * 4, np.round(v * 4)) and np.abs(v).max() < 2 ** 22      # exact in fp32, in any order
    pos = S > 0
    Sd = np.where(pos, S, 1.0)
    hc32 = np.where(pos[..., None], hc / Sd[..., None], 0.0).astype(np.float32)           # correctly rounded quotients
    h1, h2 = (np.where(pos, hs[..., i] / Sd, 0.0).astype(np.float32) for i in (0, 1))
    N = np.minimum(np.float32(history_max), (hs[..., 2] + 1.0).astype(np.float32))
    inv = (1.0 / N.astype(np.float64)).astype(np.float32)
    al, am = np.maximum(inv, np.float32(alpha)), np.maximum(inv, np.float32(alpha_moments))
    colour = fma32(al[..., None], C - hc32, hc32)                                         # C - hc: one fp32 subtraction
    l = lum32(C)
    m1 = fma32(am, l - h1, h1)
    m2 = fma32(am, l * l - h2, h2)
    v = fma32(-m1, m1, m2)
    Vt = np.where(v < 0, np.float32(0), v)
    return colour, np.stack([m1, m2, N, np.zeros_like(N)], -1), Vt, rejected / max(offered, 1)
