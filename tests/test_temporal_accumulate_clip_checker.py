"""CPU suite: the float64 checker of the accumulation with a clip box (tests/np_temporal_accumulate_clip.py, which wraps
tests/np_temporal_accumulate.py) against answers worked out by hand, and the exact evaluation
(tests/np_temporal_accumulate_clip_exact.py) against the module it restates, bit for bit."""
import numpy as np

import np_temporal_accumulate_exact as ex
import temporal_accumulate_inputs as tai
from np_atrous_variance import lum
from np_temporal_accumulate import temporal_accumulate as unclipped
from np_temporal_accumulate_clip import temporal_accumulate_clip as clipped
from np_temporal_accumulate_clip_exact import clip_planes, temporal_accumulate_clip_exact


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


H, W = 3, 4
FRAME = np.full((H, W, 4), 0.5, np.float32)
HC = np.broadcast_to(np.float32([2.0, 1.0, 0.25, 0.75]), (H, W, 4)).copy()
HS = np.broadcast_to(np.float32([1.25, 1.75, 9.0, 0.0]), (H, W, 4)).copy()      # m1 = 1.25, m2 = 1.75: the variance is 0.1875
KW = dict(alpha=0.2, alpha_moments=0.25, history_max=32, history_full=4)


def planes(lo, hi):
    return np.broadcast_to(np.float32(lo + [0]), (H, W, 4)).copy(), np.broadcast_to(np.float32(hi + [0]), (H, W, 4)).copy()


def test_a_history_above_the_box_lands_on_hi():
    """Zero motion, no layer: hc = HC, h1 = 1.25, h2 = 1.75, hn = 9, N' = 10, a = 0.2, am = 0.25.  The box [0, 1]^3 moves R from 2 to 1 and
    leaves G and B: colour = hi + 0.2 (0.5 - hi) in R, d = 0.2126 (1 - 2), m1' = h1 + d + 0.25 (l - h1 - d) with l = 0.5."""
    lo, hi = planes([0, 0, 0], [1, 1, 1])
    out = clipped(FRAME, [], [], [], hist=(HC, HS), clip_lo=lo, clip_hi=hi, **KW)
    a, am = float(np.float32(0.2)), 0.25
    want = np.array([1 + a * (0.5 - 1), 1 + a * (0.5 - 1), 0.25 + a * (0.5 - 0.25), 0.75 + a * (0.5 - 0.75)])
    assert np.allclose(out["colour"], want, rtol=1e-14) and out["clipped"][..., 0].all() and not out["clipped"][..., 1:].any()
    d = float(lum(np.array([1.0, 1.0, 0.25])) - lum(np.array([2.0, 1.0, 0.25])))      # (the checkers' luminance weights are the fp32 constants)
    assert abs(d + 0.2126) < 1e-8
    h1, h2 = 1.25 + d, 1.75 + d * (2 * 1.25 + d)
    l = float(lum(np.array([0.5, 0.5, 0.5])))
    assert np.allclose(out["state"][..., 0], h1 + am * (l - h1), rtol=1e-13, atol=0) and np.allclose(out["state"][..., 1], h2 + am * (l * l - h2), rtol=1e-13, atol=0)
    assert abs((h2 - h1 * h1) - (1.75 - 1.25 ** 2)) < 1e-15                              # the variance of the history stays 0.1875
    assert np.array_equal(out["state"][..., 2], np.full((H, W), 10.0))
    # below the box: it lands on lo
    lo, hi = planes([3, 0, 0], [4, 1, 1])
    out = clipped(FRAME, [], [], [], hist=(HC, HS), clip_lo=lo, clip_hi=hi, **KW)
    assert np.allclose(out["colour"][..., 0], 3 + a * (0.5 - 3), rtol=1e-14)


def test_inside_the_box_nan_bounds_and_no_history_weight_change_nothing():
    base = unclipped(FRAME, [], [], [], hist=(HC, HS), **KW)
    for lo, hi in (planes([0, 0, 0], [2, 1, 0.25]), planes([-np.inf] * 3, [np.inf] * 3), planes([np.nan] * 3, [np.nan] * 3), planes([-3.4e38] * 3, [3.4e38] * 3)):
        out = clipped(FRAME, [], [], [], hist=(HC, HS), clip_lo=lo, clip_hi=hi, **KW)
        assert not out["clipped"].any()
        for k in ("colour", "state", "variance"):
            assert np.allclose(out[k], base[k], rtol=1e-15, atol=1e-29), k      # (the wrap's 1e-30 blend factors)
    # S == 0: the motion points off the frame everywhere, and a box far from everything changes nothing
    away = np.full((H, W, 2), 100.0, np.float32)
    lo, hi = planes([7, 7, 7], [8, 8, 8])
    base = unclipped(FRAME, [], [], [], hist=(HC, HS), motion=away, **KW)
    out = clipped(FRAME, [], [], [], hist=(HC, HS), motion=away, clip_lo=lo, clip_hi=hi, **KW)
    assert not out["S"].any() and not out["clipped"].any()
    for k in ("colour", "state", "variance"):
        assert np.array_equal(out[k], base[k]), k
    assert np.array_equal(out["colour"], FRAME.astype(np.float64))
    # both planes None: the wrapped checker itself
    out = clipped(FRAME, [], [], [], hist=(HC, HS), **KW)
    assert all(np.array_equal(out[k], unclipped(FRAME, [], [], [], hist=(HC, HS), **KW)[k]) for k in ("colour", "state", "variance", "S"))


def test_the_clip_moves_the_mean_and_keeps_the_variance():
    """h2' - h1'^2 == h2 - h1^2: with am = 1 the state would be the frame's, so the moments are read off a call whose blend factors
    are tiny -- the history's own N = 1e6 and alpha_moments = 1e-9 -- on the recipe's inputs with real weights."""
    shape = (20, 33)
    fr, ly, pl, sg = tai.frame_of(shape, 1), tai.layers_of(shape, 3, np.uint8, 1), tai.layers_of(shape, 3, np.uint8, 0), tai.sigmas_of(3)
    col, st = tai.history_of(shape)
    st[..., 2] = 1e6
    lo, hi = np.full(shape + (4,), 0.8, np.float32), np.full(shape + (4,), 0.9, np.float32)
    kw = dict(hist=(col, st), motion=tai.motion_of(shape, "fractional"), alpha=0.2, alpha_moments=1e-9, history_max=1e9)
    a, b = unclipped(fr, ly, pl, sg, **kw), clipped(fr, ly, pl, sg, clip_lo=lo, clip_hi=hi, **kw)
    full = a["S"] > 0.5                                 # (N' = hn + 1 with hn = S * 1e6: the factors are below 2e-6 there)
    assert full.sum() > 100 and b["clipped"].any(-1)[full].mean() > 0.9
    va, vb = (o["state"][..., 1] - o["state"][..., 0] ** 2 for o in (a, b))
    moved = np.abs(b["state"][..., 0] - a["state"][..., 0])[full]
    assert moved.max() > 0.1
    assert np.abs(va - vb)[full].max() < 1e-4 * moved.max()                  # (what is left is the 2e-6 blend with the frame's moments)
    d = lum(b["colour"][..., :3]) - lum(a["colour"][..., :3])                # and the mean moved by l(hc') - l(hc), up to the blend
    assert np.allclose((b["state"][..., 0] - a["state"][..., 0])[full], d[full] / (1 - 0.2), rtol=1e-4, atol=1e-6)


def test_the_exact_evaluation_is_the_module_it_restates_where_nothing_is_clipped():
    shape = (35, 130)
    for seed, L in ((1, 0), (2, 2), (3, 4)):
        fr, hist, mv = ex.grey_frame(shape, seed), ex.history(shape, seed), ex.motion(shape, seed)
        ly, pl = ex.label_layers(shape, L, 1), ex.label_layers(shape, L, 0)
        want = ex.temporal_accumulate_exact(fr, ly, pl, hist, mv, 0.1, 0.05, 8)
        wide = np.full(shape + (4,), -np.inf, np.float32), np.full(shape + (4,), np.inf, np.float32)
        for planes_ in ((None, None), wide):
            got = temporal_accumulate_clip_exact(fr, ly, pl, hist, mv, 0.1, 0.05, 8, *planes_)
            assert all(same(g, w) for g, w in zip(got[:3], want[:3])) and got[3] == 0.0
        lo, hi = clip_planes(shape, seed)
        got = temporal_accumulate_clip_exact(fr, ly, pl, hist, mv, 0.1, 0.05, 8, lo, hi)
        assert 0.3 < got[3] < 0.98 and not same(got[0], want[0]) and same(got[1][..., 2], want[1][..., 2])
        if L:
            continue                                # (a rejected label weighs exactly 0 in fp32 and 1e-214 in float64: S > 0 differs)
        # and without layers the float64 checker agrees with it
        ref = clipped(fr, [], [], [], hist=hist, motion=mv, alpha=0.1, alpha_moments=0.05, history_max=8, clip_lo=lo, clip_hi=hi)
        # a4j's tolerance for the colour, m1 and N'.  m2: h2 + d (2 h1 + d) cancels here (integer histories whose m2 is far below
        # m1^2, terms up to 240^2 = 57600): four fp32 roundings of terms of that size, 4 x 2^-24 x 57600 = 1.4e-2, absolute
        tol = 1e-5 * np.maximum(1.0, np.abs(ref["state"]))
        tol[..., 1] = 1.4e-2
        assert (np.abs(got[0] - ref["colour"]) <= 1e-5 * np.maximum(1.0, np.abs(ref["colour"]))).all() and (np.abs(got[1] - ref["state"]) <= tol).all()
