"""The float64 checkers of layer-guided NLM (np_nlm_layers, np_nlm_layers_temporal) against a brute-force restatement of the two
contracts of include/mi_denoise.h (a4b, a4c) as plain Python loops over pixel, search offset and patch texel -- no padding, no
integral images, no threads: frames of one pixel, one row, fewer rows than the patch, windows wider than the frame, no layers,
sub-ranges of a sequence, and non-finite texels.  The GPU tests of tests/test_gpu_nlm_layers_edges.py lean on the checkers at
exactly these places."""
import math

import numpy as np
import pytest

import np_nlm_layers
import np_nlm_layers_temporal
from conftest import rel_err

TOL = 1e-12     # both sides are float64 sums of the same terms, in another order
SHAPES = [(1, 1), (1, 7), (5, 3), (9, 9), (12, 20)]
WINDOWS = {"symmetric": dict(search=(-2, 3), patch=(-1, 2)), "half_open": dict(search=(-2, 2), patch=(-1, 1)),
           "lopsided": dict(search=(-1, 4), patch=(0, 3)), "wider_than_the_frame": dict(search=(-11, 11), patch=(-1, 1))}
MAGENTA = (1.0, 0.0, 1.0, 1.0)


def brute_dispatch(gt, gn, img, hparam, search, patch):
    """One accumulate dispatch into zero sums, a4c's formula (a4b's with gt is gn): d = sum over the patch of |Gt(p+q) - Gn(p+s+q)|^2
    over rgb with texels c/255, w = exp(-d / h^2), num[p] += w * In(p+s), den[p] += w, den[p] += 0.001 once; out-of-image texels 0."""
    img = np.asarray(img)
    x = (img.astype(np.float64) / 255.0 if img.dtype == np.uint8 else img.astype(np.float64)).tolist()
    h, w = len(x), len(x[0])
    gt, gn = np.asarray(gt).astype(int).tolist(), np.asarray(gn).astype(int).tolist()
    (slo, shi), (plo, phi) = search, patch
    num = np.zeros((h, w, 4))
    den = np.zeros((h, w))
    zero = (0, 0, 0, 0)
    for py in range(h):
        for px in range(w):
            acc, accw = [0.0, 0.0, 0.0, 0.0], 0.001
            for sy in range(slo, shi):
                for sx in range(slo, shi):
                    D = 0                                   # 255^2 d, an exact integer
                    for qy in range(plo, phi):
                        for qx in range(plo, phi):
                            ty, tx, ny, nx = py + qy, px + qx, py + sy + qy, px + sx + qx
                            t = gt[ty][tx] if 0 <= ty < h and 0 <= tx < w else zero
                            n = gn[ny][nx] if 0 <= ny < h and 0 <= nx < w else zero
                            D += (t[0] - n[0]) ** 2 + (t[1] - n[1]) ** 2 + (t[2] - n[2]) ** 2
                    wt = math.exp(-(D / 65025.0) / (hparam * hparam))
                    cy, cx = py + sy, px + sx
                    if 0 <= cy < h and 0 <= cx < w:
                        c = x[cy][cx]
                        for ch in range(4):
                            acc[ch] += wt * c[ch]           # (Inf * 0 is NaN)
                    accw += wt
            num[py, px], den[py, px] = acc, accw
    return num, den


def brute_normalize(num, den):
    out = np.empty(num.shape)
    for py in range(den.shape[0]):
        for px in range(den.shape[1]):
            out[py, px] = MAGENTA if den[py, px] == 0 else num[py, px] / den[py, px]
    return out


def brute_nlm_layers(img, layers, hparam, search, patch):
    """a4b: len(layers) dispatches into zero sums, then normalize."""
    h, w = np.asarray(img).shape[:2]
    num, den = np.zeros((h, w, 4)), np.zeros((h, w))
    for g in layers:
        pn, pd = brute_dispatch(g, g, img, hparam, search, patch)
        num, den = num + pn, den + pd
    return brute_normalize(num, den)


def brute_nlm_layers_temporal(frames, layers, k, hparam, search, patch, first, count, n_layers, cache):
    """a4c: output t = for f = max(0,t-k) .. min(n-1,t+k) and inside it l = 0 .. L-1 one dispatch (Gt = layer[t][l], Gn = layer[f][l],
    In = frame[f]) into zero sums, then normalize.  cache: the sums of dispatch (t, f, l), which depend on nothing else."""
    n = len(frames)
    h, w = np.asarray(frames[0]).shape[:2]
    outs = []
    for t in range(first, first + count):
        num, den = np.zeros((h, w, 4)), np.zeros((h, w))
        for f in range(max(0, t - k), min(n - 1, t + k) + 1):
            for l in range(n_layers):
                if (t, f, l) not in cache:
                    cache[(t, f, l)] = brute_dispatch(layers[t][l], layers[f][l], frames[f], hparam, search, patch)
                num, den = num + cache[(t, f, l)][0], den + cache[(t, f, l)][1]
        outs.append(brute_normalize(num, den))
    return outs


def agree(got, want):
    """Identical NaN / +Inf / -Inf masks, and at most TOL on every other value."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    e = rel_err(got[fin], want[fin])
    assert e <= TOL, e
    return e


def data(rng, h, w, n, L):
    """n float32 frames (a few translucent texels) and per frame L RGBA8 guides a few codes apart: weights neither all 0 nor all 1."""
    base = rng.integers(0, 256, (L, h, w, 4))
    frames, layers = [], []
    for _ in range(n):
        f = rng.random((h, w, 4)).astype(np.float32)
        f[..., 3] = np.where(rng.random((h, w)) < 0.1, 0.5, 1.0)
        frames.append(f)
        layers.append([np.clip(base[l] // 8 + 100 + rng.integers(-4, 5, (h, w, 4)), 0, 255).astype(np.uint8) for l in range(L)])
    return frames, layers


@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("shape", SHAPES)
def test_nlm_layers_checker_is_the_brute_force(shape, win):
    h, w = shape
    rng = np.random.default_rng(100 * h + w + len(win))
    frames, layers = data(rng, h, w, 1, 3)
    u8 = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    for L in (0, 1, 3):
        agree(np_nlm_layers.nlm_layers(frames[0], layers[0][:L], 0.5, **WINDOWS[win]),
              brute_nlm_layers(frames[0], layers[0][:L], 0.5, **WINDOWS[win]))
    # an RGBA8 input (texels c/255) and another h; the sums themselves, which the accumulate tests compare
    agree(np_nlm_layers.nlm_layers(u8, layers[0][:1], 0.1, **WINDOWS[win]), brute_nlm_layers(u8, layers[0][:1], 0.1, **WINDOWS[win]))
    num, den = np_nlm_layers.nlm_layers_sums(frames[0], layers[0][:1], 0.5, **WINDOWS[win])
    bnum, bden = brute_dispatch(layers[0][0], layers[0][0], frames[0], 0.5, **WINDOWS[win])
    agree(num, bnum)
    agree(den, bden)


@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("shape", SHAPES)
def test_nlm_layers_temporal_checker_is_the_brute_force(shape, win):
    h, w = shape
    rng = np.random.default_rng(200 * h + w + len(win))
    frames, layers = data(rng, h, w, 4, 3)
    cache = {}
    # (k, n, L, first, count): k in {0, 1, 2}, n in {1, 3, 4}, L in {0, 1, 3}, whole sequences and sub-ranges
    for k, n, L, first, count in ((0, 1, 3, 0, 1), (1, 3, 1, 0, 3), (2, 4, 1, 1, 2), (1, 4, 0, 0, 4), (1, 4, 3, 3, 1), (2, 3, 1, 2, 1)):
        got = np_nlm_layers_temporal.nlm_layers_temporal(frames[:n], layers[:n], k, 0.5, **WINDOWS[win], first=first, count=count,
                                                         n_layers=L)
        want = brute_nlm_layers_temporal(frames[:n], layers[:n], k, 0.5, **WINDOWS[win], first=first, count=count, n_layers=L,
                                         cache=cache)
        assert len(got) == len(want) == count
        for a, b in zip(got, want):
            agree(a, b)
            assert L > 0 or (a == MAGENTA).all()


@pytest.mark.parametrize("guide", ["noisy", "step"])
def test_non_finite_texels(guide):
    # +Inf in every channel, -Inf in rgb, NaN in one channel.  "step": guides 0 | 255 at h = 0.05, where every weight is exactly 0 or 1
    # (one mismatching texel: exp(-1200) underflows in float64 too), so Inf * 0 = NaN decides which outputs are NaN and which Inf.
    h, w = 9, 12
    rng = np.random.default_rng(5)
    frames, layers = data(rng, h, w, 2, 1)
    hp = 0.5
    if guide == "step":
        g = np.zeros((h, w, 4), np.uint8)
        g[:, 6:, :3] = 255
        layers, hp = [[g], [g.copy()]], 0.05
    bad = frames[1].copy()
    bad[1, 1] = np.inf
    bad[4, 5, :3] = -np.inf
    bad[7, 9, 1] = np.nan
    win = WINDOWS["symmetric"]
    with np.errstate(all="ignore"):
        got = np_nlm_layers.nlm_layers(bad, layers[1], hp, **win)
        want = brute_nlm_layers(bad, layers[1], hp, **win)
        agree(got, want)
        assert np.isnan(want).any() and np.isposinf(want).any() and np.isneginf(want).any() and np.isfinite(want).any()
        # over frames: the non-finite texels in the neighbour only
        gt = np_nlm_layers_temporal.nlm_layers_temporal([frames[0], bad], layers, 1, hp, **win)
        wt = brute_nlm_layers_temporal([frames[0], bad], layers, 1, hp, **win, first=0, count=2, n_layers=1, cache={})
        for a, b in zip(gt, wt):
            agree(a, b)
        assert not np.isfinite(wt[0]).all()
    # what the header states: an output is non-finite exactly where its search window holds a non-finite texel, channel by channel
    slo, shi = win["search"]
    hit = np.zeros((h, w, 4), bool)
    for (y, x), chans in (((1, 1), (0, 1, 2, 3)), ((4, 5), (0, 1, 2)), ((7, 9), (1,))):
        for c in chans:
            hit[max(0, y - shi + 1):y - slo + 1, max(0, x - shi + 1):x - slo + 1, c] = True
    assert np.array_equal(~np.isfinite(want), hit)
