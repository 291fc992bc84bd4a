"""Exact answers of the accumulation with a clip box (include/mi_denoise.h, section a4m), on the construction of
tests/np_temporal_accumulate_exact.py, which is imported: grey integer frames and histories, label layers, motion in integers and
halves, and here INTEGER clip planes (multiples of 8, lo <= hi, grey or not).

The sums S, hc, h1, h2, hn are exact in fp32 in any order (that module's argument); everything after them is a fixed chain of single
fp32 operations.  The chain's new links -- step 2 of mid_temporal_accumulate_clip -- are evaluated bit-true here with that module's
fma32 and lum32:

    hc' = hc < lo ? lo : (hc > hi ? hi : hc)          comparisons and selections: exact
    d   = l(hc') - l(hc)                              two lum32 chains and one fp32 subtraction
    h1' = h1 + d                                      one fp32 addition
    h2' = fmaf(d, fmaf(2, h1, d), h2)                 two fma32

That module's temporal_accumulate_exact keeps its sums to itself, so the sums and the chain's old links are written out here once
more, in its words; tests/test_temporal_accumulate_clip_checker.py holds this file to it, bit for bit, wherever nothing is clipped.
"""
import numpy as np

from np_temporal_accumulate_exact import fma32, lum32

F32 = np.float32


def sub32(a, b):
    return (np.asarray(a, F32).astype(np.float64) - np.asarray(b, F32).astype(np.float64)).astype(F32)


def add32(a, b):
    return (np.asarray(a, F32).astype(np.float64) + np.asarray(b, F32).astype(np.float64)).astype(F32)


def clip_planes(shape, seed):
    """Integer boxes (float32 (h, w, 4) each): per channel lo in multiples of 8 from 0 to 120, hi = lo + a multiple of 8 from 0 to 120;
    the history colours are multiples of 16 from 0 to 240, so a history lies below, inside, on the edge of and above its box."""
    h, w = shape
    rng = np.random.default_rng([seed, 9])
    lo = 8.0 * rng.integers(0, 16, (h, w, 4))
    hi = lo + 8.0 * rng.integers(0, 16, (h, w, 4))
    return lo.astype(F32), hi.astype(F32)


def temporal_accumulate_clip_exact(frame, layers, prev_layers, hist, mv, alpha, alpha_moments, history_max, clip_lo=None, clip_hi=None):
    """(colour, state, Vt) as float32, bit for bit what sections a4j and a4m prescribe, and the share of pixels with a clipped channel."""
    C = np.asarray(frame, F32)
    Hc, Hs = (np.asarray(a, F32).astype(np.float64) for a in hist)
    h, w = C.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    pp = np.stack([xx, yy], -1) + np.asarray(mv, np.float64)
    assert np.array_equal(pp * 2, np.round(pp * 2))
    ok = (pp[..., 0] > -1) & (pp[..., 0] < w) & (pp[..., 1] > -1) & (pp[..., 1] < h)
    x0, y0 = np.floor(pp[..., 0]).astype(np.int64), np.floor(pp[..., 1]).astype(np.int64)
    fx, fy = pp[..., 0] - x0, pp[..., 1] - y0
    S, hc, hs = np.zeros((h, w)), np.zeros((h, w, 4)), np.zeros((h, w, 3))
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
            wt = bw[take] * same
            S[py, px] += wt
            hc[py, px] += wt[:, None] * Hc[ty, tx]
            hs[py, px] += wt[:, None] * Hs[ty, tx, :3]
    for v in (S, hc, hs):
        assert np.array_equal(v * 4, np.round(v * 4)) and np.abs(v).max() < 2 ** 22
    pos = S > 0
    Sd = np.where(pos, S, 1.0)
    hc32 = np.where(pos[..., None], hc / Sd[..., None], 0.0).astype(F32)
    h1, h2 = (np.where(pos, hs[..., i] / Sd, 0.0).astype(F32) for i in (0, 1))
    share = 0.0
    if clip_lo is not None:
        lo, hi = np.asarray(clip_lo, F32)[..., :3], np.asarray(clip_hi, F32)[..., :3]
        rgb = hc32[..., :3]
        cl = np.where(rgb < lo, lo, np.where(rgb > hi, hi, rgb))
        cl = np.where(pos[..., None], cl, rgb)
        d = sub32(lum32(cl), lum32(rgb))
        h2 = fma32(d, fma32(F32(2), h1, d), h2)
        h1 = add32(h1, d)
        share = float((cl != rgb).any(-1).mean())
        hc32 = np.concatenate([cl, hc32[..., 3:]], -1)
    N = np.minimum(F32(history_max), (hs[..., 2] + 1.0).astype(F32))
    inv = (1.0 / N.astype(np.float64)).astype(F32)
    al, am = np.maximum(inv, F32(alpha)), np.maximum(inv, F32(alpha_moments))
    colour = fma32(al[..., None], C - hc32, hc32)
    l = lum32(C)
    m1 = fma32(am, l - h1, h1)
    m2 = fma32(am, l * l - h2, h2)
    v = fma32(-m1, m1, m2)
    Vt = np.where(v < 0, F32(0), v)
    return colour, np.stack([m1, m2, N, np.zeros_like(N)], -1), Vt, share
