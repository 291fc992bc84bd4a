"""The float64 checker of joint layer-guided NLM (np_nlm_joint) against a brute-force restatement of section a4f of
include/mi_denoise.h as plain Python loops over pixel, neighbour frame, search offset, layer and patch texel -- no padding, no box
sums, no threads, a layer's patch distance an exact Python integer: frames of one pixel, one row, fewer rows than the patch, windows
wider than the frame, one to three layers with UNEQUAL h (a ratio of 2500 among them), sequences with k = 0, 1, 2 and a sub-range,
and non-finite texels.  The GPU tests of tests/test_gpu_nlm_joint_edges.py lean on the checker at exactly these places; until
now it was anchored through its one-layer case and two hand answers with equal h."""
import math

import numpy as np
import pytest

import np_nlm_joint as chk
from conftest import rel_err

# (the checker shares the search offsets out over threads, and NumPy's error state is per thread: np.errstate does not reach them)
pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")

TOL = 1e-12     # both sides are float64 sums of the same terms, in another order
SHAPES = [(1, 1), (1, 7), (5, 3), (9, 9), (12, 20)]
WINDOWS = {"symmetric": ((-2, 3), (-1, 2)), "half_open": ((-2, 2), (-1, 1)), "lopsided": ((-1, 4), (0, 3)),
           "wider_than_the_frame": ((-11, 11), (-1, 1))}
MAGENTA = (1.0, 0.0, 1.0, 1.0)
HS3 = (0.3, 1.0, 0.1)


def brute_distances(gt, gn, search, patch):
    """D[py][px][s] = 255^2 d_l(p, f, s) of ONE layer: the patch sum of |Gt(p+q) - Gn(p+s+q)|^2 over rgb in byte values, an exact
    Python integer; out-of-image texels are 0; s counts the offsets row by row."""
    gt, gn = np.asarray(gt).astype(int).tolist(), np.asarray(gn).astype(int).tolist()
    h, w = len(gt), len(gt[0])
    (slo, shi), (plo, phi) = search, patch
    zero = (0, 0, 0, 0)
    out = []
    for py in range(h):
        row = []
        for px in range(w):
            per_offset = []
            for sy in range(slo, shi):
                for sx in range(slo, shi):
                    D = 0
                    for qy in range(plo, phi):
                        ty, ny = py + qy, py + sy + qy
                        trow = gt[ty] if 0 <= ty < h else None          # (None: the whole row lies outside the image)
                        nrow = gn[ny] if 0 <= ny < h else None
                        for qx in range(plo, phi):
                            tx, nx = px + qx, px + sx + qx
                            t = trow[tx] if trow is not None and 0 <= tx < w else zero
                            n = nrow[nx] if nrow is not None and 0 <= nx < w else zero
                            D += (t[0] - n[0]) ** 2 + (t[1] - n[1]) ** 2 + (t[2] - n[2]) ** 2
                    per_offset.append(D)
            row.append(per_offset)
        out.append(row)
    return out


def brute_pair(D, img, hs, search):
    """One neighbour frame's sums: w = exp(-sum_l d_l / h_l^2) with d_l = D[l] / 255^2, num[p] = sum_s w In(p+s), den[p] = 0.001 +
    sum_s w.  D: one brute_distances per layer."""
    img = np.asarray(img)
    x = (img.astype(np.float64) / 255.0 if img.dtype == np.uint8 else img.astype(np.float64)).tolist()
    h, w = len(x), len(x[0])
    slo, shi = search
    num = np.zeros((h, w, 4))
    den = np.zeros((h, w))
    for py in range(h):
        for px in range(w):
            acc, accw, s = [0.0, 0.0, 0.0, 0.0], 0.001, 0
            for sy in range(slo, shi):
                for sx in range(slo, shi):
                    arg = 0.0
                    for l, hl in enumerate(hs):
                        arg += (D[l][py][px][s] / 65025.0) / (hl * hl)
                    wt = math.exp(-arg)
                    cy, cx = py + sy, px + sx
                    if 0 <= cy < h and 0 <= cx < w:
                        c = x[cy][cx]
                        for ch in range(4):
                            acc[ch] += wt * c[ch]           # (Inf * 0 is NaN)
                    accw += wt
                    s += 1
            num[py, px], den[py, px] = acc, accw
    return num, den


def brute_nlm_joint(frames, layers, hs, k, search, patch, first, count, cache):
    """a4f: output t = sum over f = max(0,t-k) .. min(n-1,t+k) of the pair sums, normalized (magenta where the denominator is 0).
    cache: the integer distances of (t, f, l), which depend on neither h nor k."""
    n = len(frames)
    h, w = np.asarray(frames[0]).shape[:2]
    outs = []
    for t in range(first, first + count):
        num, den = np.zeros((h, w, 4)), np.zeros((h, w))
        for f in range(max(0, t - k), min(n - 1, t + k) + 1):
            for l in range(len(hs)):
                if (t, f, l) not in cache:
                    cache[(t, f, l)] = brute_distances(layers[t][l], layers[f][l], search, patch)
            pn, pd = brute_pair([cache[(t, f, l)] for l in range(len(hs))], frames[f], hs, search)
            num, den = num + pn, den + pd
        out = np.empty((h, w, 4))
        for py in range(h):
            for px in range(w):
                out[py, px] = MAGENTA if den[py, px] == 0 else num[py, px] / den[py, px]
        outs.append(out)
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
    """n float32 frames (a few translucent texels) and per frame L RGBA8 guides a few codes apart: weights neither all 0 nor all 1
    at h = 0.1 .. 1."""
    base = rng.integers(0, 256, (L, h, w, 4))
    frames, layers = [], []
    for _ in range(n):
        f = rng.random((h, w, 4)).astype(np.float32)
        f[..., 3] = np.where(rng.random((h, w)) < 0.1, 0.5, 1.0)
        frames.append(f)
        layers.append([np.clip(base[l] // 8 + 100 + rng.integers(-4, 5, (h, w, 4)), 0, 255).astype(np.uint8) for l in range(L)])
    return frames, layers


# (L, hs, k, first, count) on three frames: every L, every k, whole sequences and the sub-range first = 1, count = 1; the ratio
# h_0 / h_1 = 2500 in both directions
CONFIGS = ((1, HS3[:1], 0, 0, 3), (2, HS3[:2], 1, 0, 3), (3, HS3, 2, 0, 3), (3, HS3, 1, 1, 1), (2, (50.0, 0.02), 1, 1, 1),
           (2, (0.02, 50.0), 2, 1, 1), (1, (0.1,), 2, 1, 1))
# the window wider than the frame costs 484 offsets a pixel: there only output 1, whose neighbours at k >= 1 are all three frames
CONFIGS_WIDE = ((2, (50.0, 0.02), 1, 1, 1), (3, HS3, 0, 1, 1), (1, (0.1,), 2, 1, 1))


@pytest.mark.parametrize("win", list(WINDOWS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nlm_joint_checker_is_the_brute_force(shape, win):
    h, w = shape
    search, patch = WINDOWS[win]
    rng = np.random.default_rng(300 * h + w + len(win))
    frames, layers = data(rng, h, w, 3, 3)
    cache = {}
    weighed = 0
    for L, hs, k, first, count in (CONFIGS_WIDE if win == "wider_than_the_frame" else CONFIGS):
        ls = [g[:L] for g in layers]
        got = chk.nlm_joint(frames, ls, hs, k, search, patch, first=first, count=count)
        want = brute_nlm_joint(frames, ls, hs, k, search, patch, first, count, cache)
        assert len(got) == len(want) == count
        for a, b in zip(got, want):
            agree(a, b)
        weighed += sum(int((np.abs(b - frames[first + i]) > 1e-3).sum()) for i, b in enumerate(want))
    # the guides are not degenerate: some output is more than its own centre texel (which a weight sum of 1.001 would leave)
    assert weighed > 0 or shape == (1, 1)
    # an RGBA8 frame: texels c / 255
    u8 = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(3)]
    agree(chk.nlm_joint(u8, [g[:2] for g in layers], (0.3, 0.6), 1, search, patch, first=1, count=1)[0],
          brute_nlm_joint(u8, [g[:2] for g in layers], (0.3, 0.6), 1, search, patch, 1, 1, cache)[0])


@pytest.mark.parametrize("L", [1, 2, 3])
def test_non_finite_texels(L):
    # +Inf in every channel, -Inf in rgb, NaN in one colour channel, NaN in alpha alone.  Guides of 0 and 255 only at unequal
    # h <= 0.05: one mismatching texel gives at most exp(-1200), 0 in float64, so every weight is exactly 0 or 1 and Inf * 0 = NaN
    # decides which outputs are NaN and which Inf.
    h, w = 9, 12
    search, patch = WINDOWS["symmetric"]
    rng = np.random.default_rng(6)
    frames, _ = data(rng, h, w, 2, 1)
    gx = np.zeros((h, w, 4), np.uint8)
    gx[:, 6:, :3] = 255                 # a step in x
    gy = np.zeros((h, w, 4), np.uint8)
    gy[4:, :, :3] = 255                 # a step in y
    layers = [[gx, gy, gx][:L], [gx.copy(), gy.copy(), gx.copy()][:L]]
    hs = (0.05, 0.03, 0.04)[:L]
    bad = frames[1].copy()
    bad[1, 1] = np.inf
    bad[4, 5, :3] = -np.inf
    bad[7, 9, 1] = np.nan
    bad[2, 9, 3] = np.nan
    with np.errstate(all="ignore"):
        got = chk.nlm_joint([bad], layers[1:], hs, 0, search, patch)[0]
        want = brute_nlm_joint([bad], layers[1:], hs, 0, search, patch, 0, 1, {})[0]
        agree(got, want)
        assert np.isnan(want).any() and np.isposinf(want).any() and np.isneginf(want).any() and np.isfinite(want).any()
        # over frames: the non-finite texels in the neighbour only
        gt = chk.nlm_joint([frames[0], bad], layers, hs, 1, search, patch)
        wt = brute_nlm_joint([frames[0], bad], layers, hs, 1, search, patch, 0, 2, {})
        for a, b in zip(gt, wt):
            agree(a, b)
        assert not np.isfinite(wt[0]).all()
    # what the header states ("by IEEE arithmetic"): an output is non-finite exactly where its search window holds a non-finite
    # texel, channel by channel -- a weight of 0 makes it NaN, a weight of 1 keeps its sign
    slo, shi = search
    hit = np.zeros((h, w, 4), bool)
    for (y, x), chans in (((1, 1), (0, 1, 2, 3)), ((4, 5), (0, 1, 2)), ((7, 9), (1,)), ((2, 9), (3,))):
        for c in chans:
            hit[max(0, y - shi + 1):y - slo + 1, max(0, x - shi + 1):x - slo + 1, c] = True
    assert np.array_equal(~np.isfinite(want), hit)


def test_unequal_h_is_not_equal_h():
    """The layers' h enter one by one: swapping two unequal h changes the result, and the brute force follows the checker there."""
    h, w = 9, 9
    search, patch = WINDOWS["symmetric"]
    rng = np.random.default_rng(7)
    frames, layers = data(rng, h, w, 1, 2)
    a = chk.nlm_joint(frames, layers, (0.3, 1.0), 0, search, patch)[0]
    b = chk.nlm_joint(frames, layers, (1.0, 0.3), 0, search, patch)[0]
    assert rel_err(a, b) > 1e-3
    agree(b, brute_nlm_joint(frames, layers, (1.0, 0.3), 0, search, patch, 0, 1, {})[0])
