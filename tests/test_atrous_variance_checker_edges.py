"""CPU: the vectorised float64 checker of the variance-guided a-trous filter (np_atrous_variance.py) at the edges of its domain,
against plain per-pixel loops written from the text of include/mi_denoise.h, section a4i: one `for` per pixel, one per tap, a tap
outside the image is skipped.  Frames smaller than the tap pattern, steps at which every off-centre tap lies outside, 1 x 1, one
to three layers with unequal sigmas, sigma_lum 0 and 4, the moments at k = 0, 1, 2 for every t, and non-finite texels: the GPU
tests of the edges (test_gpu_atrous_variance_edges.py) rest on the checker being right exactly there.  Agreement: 1e-12 max(1, |ref|).
"""
import math

import numpy as np
import pytest

import np_atrous_variance as chk
from np_atrous_joint import widen

SHAPES = [(1, 1), (1, 5), (5, 1), (2, 3), (5, 7), (7, 3), (9, 11)]
STEPS = (1, 2, 4, 8)
SIGMAS = (0.3, 0.7, 0.45)
K = (1 / 16, 4 / 16, 6 / 16, 4 / 16, 1 / 16)
G3 = (0.25, 0.5, 0.25)
LR, LG, LB = (float(np.float32(c)) for c in (0.2126, 0.7152, 0.0722))
TOL = 1e-12


def _frame(shape, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.gamma(4.0, 0.25, shape + (3,)), rng.random(shape + (1,))], -1).astype(np.float32)


def _layers(shape, L, seed):
    rng = np.random.default_rng(seed)
    return [rng.random(shape + (4,)).astype(np.float32) for _ in range(L)]


def _lum(c):
    return LR * c[0] + LG * c[1] + LB * c[2]


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else float("nan")         # (false for a NaN too)


def loop_vt(V, y, x):
    h, w = len(V), len(V[0])
    num = den = 0.0
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            yy, xx = y + j, x + i
            if yy < 0 or yy >= h or xx < 0 or xx >= w:
                continue
            g = G3[j + 1] * G3[i + 1]
            num += g * V[yy][xx]
            den += g
    return num / den


def loop_pass(C, V, layers, sigmas, step, sigma_lum, epsilon):
    """One pass by the header's text on nested lists of Python floats: C [h][w][4], V [h][w], layers [l][h][w][3]."""
    h, w = len(V), len(V[0])
    outC = [[None] * w for _ in range(h)]
    outV = [[None] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            if sigma_lum > 0:
                inv = 1.0 / (sigma_lum * _sqrt(loop_vt(V, y, x)) + epsilon)
                lp = _lum(C[y][x])
            acc, accw, accv = [0.0] * 4, 0.0, 0.0
            for j in range(-2, 3):
                for i in range(-2, 3):
                    yy, xx = y + j * step, x + i * step
                    if yy < 0 or yy >= h or xx < 0 or xx >= w:
                        continue
                    arg = 0.0
                    for g, s in zip(layers, sigmas):
                        arg -= 0.5 * sum((g[y][x][c] - g[yy][xx][c]) ** 2 for c in range(3)) / (s * s)
                    if sigma_lum > 0:
                        arg -= abs(lp - _lum(C[yy][xx])) * inv
                    wt = K[i + 2] * K[j + 2] * math.exp(arg)
                    for c in range(4):
                        acc[c] += wt * C[yy][xx][c]
                    accw += wt
                    accv += wt * wt * V[yy][xx]
            outC[y][x] = [a / accw for a in acc]
            outV[y][x] = accv / (accw * accw)
    return np.array(outC), np.array(outV)


def loop_moments(frames, layers, sigmas, k, t):
    """(V_0, M2) by the header's text; frames [f][h][w][4], layers [f][l][h][w][3]."""
    n, h, w = len(frames), len(frames[0]), len(frames[0][0])
    V0, M2 = np.empty((h, w)), np.empty((h, w))
    for y in range(h):
        for x in range(w):
            lp = _lum(frames[t][y][x])
            W = s1 = s2 = 0.0
            for f in range(max(0, t - k), min(n - 1, t + k) + 1):
                for j in range(-3, 4):
                    for i in range(-3, 4):
                        yy, xx = y + j, x + i
                        if yy < 0 or yy >= h or xx < 0 or xx >= w:
                            continue
                        arg = 0.0
                        for l, s in enumerate(sigmas):
                            arg -= 0.5 * sum((layers[t][l][y][x][c] - layers[f][l][yy][xx][c]) ** 2 for c in range(3)) / (s * s)
                        wt = math.exp(arg)
                        d = _lum(frames[f][yy][xx]) - lp
                        W += wt
                        s1 += wt * d
                        s2 += wt * d * d
            m, m2 = s1 / W, s2 / W
            v = m2 - m * m
            V0[y, x], M2[y, x] = (0.0 if v < 0 else v), m2
    return V0, M2


def lists(a):
    return widen(a).tolist()


def agree(got, want):
    """Equal non-finite masks, and the finite values within TOL max(1, |want|)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = ~np.isfinite(want)
    if not np.array_equal(~np.isfinite(got), bad):
        return False
    return bool(np.all(np.abs(got[~bad] - want[~bad]) <= TOL * np.maximum(1.0, np.abs(want[~bad]))))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_pass_and_the_smoothed_variance_at_every_step(shape):
    si = SHAPES.index(shape)
    h, w = shape
    for step, L in ((s, n) for s in STEPS for n in (1, 2, 3)):
        fr, ly, sg = _frame(shape, 10 + si), _layers(shape, L, 20 + si + L), list(SIGMAS[:L])
        V = np.random.default_rng(30 + si).gamma(2.0, 0.2, shape)
        Gs = np.concatenate([widen(g)[..., :3] / s for g, s in zip(ly, sg)], -1)
        none_inside = step >= max(h, w)                      # a tap (i, j) != (0, 0) needs |i| step < w and |j| step < h
        for sl in (0.0, 4.0):
            gotC, gotV = chk.one_pass(widen(fr), V, Gs, step, sl, 1e-3)
            wantC, wantV = loop_pass(lists(fr), V.tolist(), [lists(g[..., :3]) for g in ly], sg, step, sl, 1e-3)
            assert agree(gotC, wantC) and agree(gotV, wantV), (shape, step, L, sl)
            if none_inside:                                  # every off-centre tap lies outside: the pass is the identity
                assert agree(gotC, widen(fr)) and agree(gotV, V), (shape, step)
        vt = chk.smooth_variance(V)
        assert agree(vt, [[loop_vt(V.tolist(), y, x) for x in range(w)] for y in range(h)]), shape


def test_the_whole_filter_is_the_chain_of_its_passes():
    shape = (5, 7)
    fr, ly, sg = _frame(shape, 1), _layers(shape, 2, 2), [0.3, 0.7]
    V = np.random.default_rng(3).gamma(2.0, 0.2, shape).astype(np.float32)
    C, Vl = lists(fr), V.astype(np.float64).tolist()
    for i in range(2, 5):
        C, Vl = (a.tolist() for a in loop_pass(C, Vl, [lists(g[..., :3]) for g in ly], sg, 2 ** i, 4.0, 1e-3))
    gotC, gotV = chk.atrous_variance(fr, V, ly, sg, passes=3, first_pass=2, sigma_lum=4.0, epsilon=1e-3)
    assert agree(gotC, C) and agree(gotV, Vl)


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (9, 11)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_for_every_window(shape):
    n = 4
    for k in (0, 1, 2):
        L = k + 1
        fr = [_frame(shape, 40 + f) for f in range(n)]
        ly = [_layers(shape, L, 50 + 7 * f + k) for f in range(n)]
        sg = list(SIGMAS[:L])
        for t in range(n):
            got = chk.moments(fr, ly, sg, k=k, t=t)
            want = loop_moments([lists(f) for f in fr], [[lists(g[..., :3]) for g in ls] for ls in ly], sg, k, t)
            assert agree(got[0], want[0]) and agree(got[1], want[1]), (shape, k, t)
            assert got[0].min() >= 0


@pytest.mark.parametrize("step", [1, 2, 8])
def test_non_finite_texels_reach_the_same_pixels(step):
    shape = (9, 11)
    fr, ly, sg = _frame(shape, 60), _layers(shape, 2, 61), [0.3, 0.7]
    V = np.random.default_rng(62).gamma(2.0, 0.2, shape)
    fr[2, 3, 1] = np.nan
    fr[6, 8, 0] = np.inf
    V[7, 1] = np.nan
    V[1, 9] = -5.0
    Gs = np.concatenate([widen(g)[..., :3] / s for g, s in zip(ly, sg)], -1)
    gotC, gotV = chk.one_pass(widen(fr), V, Gs, step, 4.0, 1e-3)
    wantC, wantV = loop_pass(lists(fr), V.tolist(), [lists(g[..., :3]) for g in ly], sg, step, 4.0, 1e-3)
    assert agree(gotC, wantC) and agree(gotV, wantV)
    bad = ~np.isfinite(gotC).all(-1) | ~np.isfinite(gotV)
    assert bad[2, 3] and bad[6, 8] and bad[7, 1] and bad[1, 9] and 4 < bad.sum() < bad.size
    assert np.isnan(chk.smooth_variance(V)[7, 1]) and chk.smooth_variance(V)[1, 9] < 0       # sqrt of a negative vt: a NaN scale
    # the moments: a NaN and an Inf luminance
    frames = [fr, _frame(shape, 63)]
    layers = [ly, _layers(shape, 2, 64)]
    got = chk.moments(frames, layers, sg, k=1, t=1)
    want = loop_moments([lists(f) for f in frames], [[lists(g[..., :3]) for g in ls] for ls in layers], sg, 1, 1)
    assert agree(got[0], want[0]) and np.isnan(got[0]).sum() >= 2 * 16
