"""CPU suite: the float64 checker of the image metrics (tests/np_image_metrics.py, section a4n) held to three things before any GPU
test trusts it: (a) per-pixel Python loops written from the header on frames of 1 x 1 .. 13 x 13 with non-finite texels, (b) an
independent evaluation of the interior by scipy.ndimage.correlate1d with the same six constants, (c) answers worked out by hand."""
import math

import numpy as np
import pytest
from scipy.ndimage import correlate1d

import np_image_metrics as M
from image_metrics_inputs import as_dtype, pair
from np_albedo import widen
from np_temporal_accumulate_exact import lum32


def loops(a, b, peak, eps):
    """The header, pixel by pixel and tap by tap."""
    A, B = widen(a), widen(b)
    la, lb = lum32(A).astype(np.float64), lum32(B).astype(np.float64)
    A, B = A[..., :3].astype(np.float64), B[..., :3].astype(np.float64)
    h, w = la.shape
    g = [math.exp(-k * k / 4.5) for k in range(6)]
    c1, c2 = (0.01 * peak) ** 2, (0.03 * peak) ** 2
    valid = [[all(math.isfinite(v) for v in A[y, x]) and all(math.isfinite(v) for v in B[y, x]) for x in range(w)] for y in range(h)]
    sums = [0.0] * 16
    smap = np.full((h, w), np.nan)
    for y in range(h):
        for x in range(w):
            if not valid[y][x]:
                sums[1] += 1
                continue
            sums[0] += 1
            for c in range(3):
                d = A[y, x, c] - B[y, x, c]
                sums[2 + c] += d * d
                sums[5 + c] += abs(d)
                sums[8] = max(sums[8], abs(d))
                sums[9 + c] += d * d / (B[y, x, c] ** 2 + eps)
            W = sa = sb = saa = sbb = sab = 0.0
            for j in range(-5, 6):
                for i in range(-5, 6):
                    qy, qx = y + j, x + i
                    if not (0 <= qy < h and 0 <= qx < w) or not valid[qy][qx]:
                        continue
                    wq = g[abs(i)] * g[abs(j)]
                    W += wq
                    sa += wq * la[qy, qx]
                    sb += wq * lb[qy, qx]
                    saa += wq * la[qy, qx] ** 2
                    sbb += wq * lb[qy, qx] ** 2
                    sab += wq * la[qy, qx] * lb[qy, qx]
            ma, mb = sa / W, sb / W
            s = (2 * ma * mb + c1) * (2 * (sab / W - ma * mb) + c2) / ((ma * ma + mb * mb + c1) * (saa / W - ma * ma + sbb / W - mb * mb + c2))
            smap[y, x] = s
            sums[12] += s
    return np.array(sums), smap


@pytest.mark.parametrize("size", [(1, 1), (1, 2), (2, 3), (5, 5), (6, 11), (11, 6), (12, 12), (13, 13), (13, 4)])
def test_checker_against_per_pixel_loops(size):
    h, w = size
    a, b = pair(h, w, scale=3.0, seed=h * 31 + w)
    rng = np.random.default_rng(h * 100 + w)
    if h * w > 1:                                   # non-finite texels: in a, in b, in both; a non-finite ALPHA does not count
        for k, bad in enumerate((np.nan, np.inf, -np.inf)):
            y, x, c = rng.integers(h), rng.integers(w), rng.integers(3)
            (a, b, a)[k][y, x, c] = bad
        b[0, 0, 1] = np.nan
        a[0, 0, 2] = np.inf
        a[h - 1, w - 1, 3] = np.nan
    got = M.image_metrics(a, b, peak=3.0, eps=0.05)
    sums, smap = loops(a, b, 3.0, float(np.float32(0.05)))
    assert got["sums"][0] == sums[0] and got["sums"][1] == sums[1] and got["sums"][8] == sums[8]
    assert got["sums"][0] + got["sums"][1] == h * w and (h * w == 1 or got["sums"][1] >= 1)
    np.testing.assert_allclose(got["sums"], sums, rtol=1e-13, atol=0)
    assert np.array_equal(np.isnan(got["map"]), np.isnan(smap)) and np.array_equal(np.isnan(smap), ~got["valid"])
    np.testing.assert_allclose(got["map"][got["valid"]], smap[got["valid"]], rtol=0, atol=1e-11)


@pytest.mark.parametrize("dtypes", [(np.float32, np.float32), (np.uint8, np.float16)])
def test_checker_interior_against_scipy(dtypes):
    h, w = 29, 37
    a, b = pair(h, w)
    a, b = as_dtype(a, dtypes[0]), as_dtype(b, dtypes[1])
    got = M.image_metrics(a, b)
    la, lb = lum32(widen(a)).astype(np.float64), lum32(widen(b)).astype(np.float64)
    k = np.array([M.G[abs(i)] for i in range(-5, 6)])

    def blur(x):
        return correlate1d(correlate1d(x, k, axis=1, mode="constant"), k, axis=0, mode="constant") / k.sum() ** 2

    ma, mb = blur(la), blur(lb)
    saa, sbb, sab = blur(la * la) - ma * ma, blur(lb * lb) - mb * mb, blur(la * lb) - ma * mb
    c1, c2 = 1e-4, 9e-4
    s = (2 * ma * mb + c1) * (2 * sab + c2) / ((ma * ma + mb * mb + c1) * (saa + sbb + c2))
    np.testing.assert_allclose(got["map"][5:-5, 5:-5], s[5:-5, 5:-5], rtol=0, atol=1e-11)
    assert got["map"][5:-5, 5:-5].size == 19 * 27


def test_hand_answers():
    h, w = 9, 14
    one = np.ones((h, w, 1), np.float32)

    def const(c):
        return np.concatenate([np.full((h, w, 3), c, np.float32), one], -1)

    # two constant images: every moment is the constant's, S_.. = 0, whatever part of the window is missing -- corners included
    for c1_, c2_, peak in ((0.25, 0.75, 1.0), (0.5, 0.5, 1.0), (100.0, 7.0, 255.0), (0.0, 1.0, 1.0)):
        r = M.image_metrics(const(c1_), const(c2_), peak=peak)
        la, lb = float(lum32(const(c1_))[0, 0]), float(lum32(const(c2_))[0, 0])
        C1 = (0.01 * peak) ** 2
        want = (2 * la * lb + C1) / (la * la + lb * lb + C1)
        assert np.abs(r["map"] - want).max() <= 1e-12, (c1_, c2_, np.abs(r["map"] - want).max())
        assert abs(r["ssim"] - want) <= 1e-12
        d = float(np.float32(c1_)) - float(np.float32(c2_))
        assert r["mse"] == pytest.approx(d * d, rel=1e-15) and r["mae"] == pytest.approx(abs(d), rel=1e-15) and r["max_abs"] == abs(d)
    # a == b: exactly 1 everywhere, every error sum +0, psnr +Inf
    a, _ = pair(h, w, scale=5.0)
    r = M.image_metrics(a, a, peak=5.0)
    assert np.array_equal(r["map"], np.ones((h, w))) and r["ssim"] == 1.0 and r["sums"][12] == h * w
    assert not r["sums"][2:12].any() and r["mse"] == 0 and r["psnr"] == math.inf and r["relmse"] == 0
    # b = 0, a = c: relMSE is c^2 / eps in closed form
    r = M.image_metrics(const(0.5), const(0.0), eps=0.25)
    assert r["relmse"] == 1.0 and r["mse"] == 0.25
    # one level of an 8-bit image everywhere: psnr = 20 log10(255) with peak 1 on c / 255, and with peak 255 on integer levels
    u = np.full((h, w, 4), 100, np.uint8)
    v = u.copy()
    v[..., :3] += 1
    assert M.image_metrics(v.astype(np.float32), u.astype(np.float32), peak=255.0)["psnr"] == pytest.approx(20 * math.log10(255), abs=1e-12)
    assert M.image_metrics(v, u)["psnr"] == pytest.approx(20 * math.log10(255), abs=1e-5)       # c / 255 is rounded to float32
    # nothing valid: the counts, zero sums, NaN ratios
    r = M.image_metrics(const(np.nan), const(1.0))
    assert r["n_valid"] == 0 and r["n_invalid"] == h * w and not r["sums"][2:].any() and np.isnan(r["map"]).all()
    assert all(math.isnan(r[k]) for k in ("mse", "mse_r", "mae", "psnr", "relmse", "ssim")) and r["max_abs"] == 0


def test_tolerances_are_the_stated_ones():
    assert M.sum_rtol(100) == 108 * 2.0 ** -53 * 8
    assert M.ssim_atol(2.0, 4.0) == 1e-12 + 1e-10 * 0.25
