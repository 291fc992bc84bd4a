"""GPU suite: mid_image_metrics (section a4n) against its float64 checker (tests/np_image_metrics.py) on the recipe of
tests/image_metrics_inputs.py: frames from 1 x 1 past both tile seams, every height 1 .. 34 at width 67, every pair of formats,
ssim off / on / with the map, radiance from 1/64 to 1024 with the peak scaled alike.

Tolerances, derived in the header and not from what the kernel gives (np_image_metrics.sum_rtol / ssim_atol):
    n_valid, n_invalid, max |d|     bit for bit
    every sum                       relative (n + 8) 2^-53 8 -- the terms are >= 0 and each carries at most three roundings
    ssim(p)                         1e-12 + 1e-10 (M(p) / peak)^2, M the largest |l| of the window; the mean with the frame's largest M
    map                             that bound plus one fp32 rounding
"""
import functools

import numpy as np
import pytest

import np_image_metrics as M
from image_metrics_inputs import DTYPES, SHAPES, as_dtype, pair

pytestmark = pytest.mark.gpu
PAIRS = [(da, db) for da in DTYPES for db in DTYPES]
worst = {"sum": 0.0, "ssim": 0.0, "mean": 0.0, "map": 0.0}         # the largest error seen, as a fraction of its tolerance


@functools.lru_cache(maxsize=None)
def frames(h, w, da, db, scale=1.0):
    a, b = pair(h, w, scale)
    if scale == 1.0:
        a, b = as_dtype(a, da), as_dtype(b, db)
    else:
        a, b = a.astype(da), b.astype(db)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def reference(h, w, da, db, scale=1.0):
    a, b = frames(h, w, da, db, scale)
    return M.image_metrics(a, b, peak=scale, eps=1e-2 * scale * scale)


def holds(got, ref, peak, ssim, want_map):
    """One call's result against the checker's, to the stated tolerances."""
    s, r = got["sums"], ref["sums"]
    n = r[M.I_VALID]
    assert s[M.I_VALID] == n and s[M.I_INVALID] == r[M.I_INVALID] and s[M.I_MAX] == r[M.I_MAX]
    assert not s[13:].any()
    for i in list(range(2, 8)) + [9, 10, 11]:
        e = abs(s[i] - r[i])
        assert e <= M.sum_rtol(n) * r[i], (i, s[i], r[i])
        if r[i]:
            worst["sum"] = max(worst["sum"], e / (M.sum_rtol(n) * r[i]))
    for k in ("n_valid", "n_invalid", "max_abs"):
        assert got[k] == ref[k]
    if not ssim:
        assert s[M.I_SSIM] == 0 and np.isnan(got["ssim"]) and "map" not in got
        return
    if n:
        tol = float(M.ssim_atol(ref["M"].max(), peak))
        e = abs(s[M.I_SSIM] / n - ref["sums"][M.I_SSIM] / n)
        assert e <= tol, (s[M.I_SSIM] / n, ref["sums"][M.I_SSIM] / n, tol)
        worst["mean"] = max(worst["mean"], e / tol)
    if want_map:
        m = got["map"]
        assert m.dtype == np.float32 and m.shape == ref["map"].shape
        assert np.array_equal(np.isnan(m), ~ref["valid"])
        v = ref["valid"]
        e = np.abs(m[v].astype(np.float64) - ref["map"][v])
        tol = M.ssim_atol(ref["M"][v], peak) + np.abs(ref["map"][v]) * 2.0 ** -24
        assert (e <= tol).all(), float((e / tol).max())
        if v.any():
            worst["map"] = max(worst["map"], float((e / tol).max()))
            # (the binary64 value itself is not returned per pixel: the part of the map's error that is not fp32 rounding)
            worst["ssim"] = max(worst["ssim"], float((np.maximum(e - np.abs(ref["map"][v]) * 2.0 ** -24, 0) / M.ssim_atol(ref["M"][v], peak)).max()))


def three_ways(ctx, a, b, ref, peak=1.0, eps=1e-2):
    """ssim off, on, and with the map: each against the checker, and the three against each other bit for bit."""
    full = ctx.image_metrics(a, b, peak=peak, eps=eps, ssim=True, want_map=True)
    holds(full, ref, peak, True, True)
    plain = ctx.image_metrics(a, b, peak=peak, eps=eps, ssim=True, want_map=False)
    holds(plain, ref, peak, True, False)
    assert plain["sums"].tobytes() == full["sums"].tobytes()                # the map changes no sum
    off = ctx.image_metrics(a, b, peak=peak, eps=eps, ssim=False)
    holds(off, ref, peak, False, False)
    assert off["sums"][:12].tobytes() == full["sums"][:12].tobytes()        # ssim == 0: the pointwise sums of ssim == 1
    return full


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_every_pair_of_formats(ctx, shape):
    h, w = shape
    for da, db in PAIRS:
        a, b = frames(h, w, da, db)
        three_ways(ctx, a, b, reference(h, w, da, db))
    print(f"{w}x{h}: worst fractions of the tolerances so far {worst}")


@pytest.mark.parametrize("h", range(1, 35))
def test_every_height_at_width_67(ctx, h):
    da, db = PAIRS[h % len(PAIRS)]
    a, b = frames(h, 67, da, db)
    three_ways(ctx, a, b, reference(h, 67, da, db))


@pytest.mark.parametrize("scale", [1 / 64, 1 / 3, 5.5, 1024.0])
@pytest.mark.parametrize("dt", [np.float16, np.float32], ids=["f16", "f32"])
def test_radiance_scaled_with_the_peak(ctx, scale, dt):
    h, w = 33, 129
    a, b = frames(h, w, dt, np.float32, scale)
    three_ways(ctx, a, b, reference(h, w, dt, np.float32, scale), peak=scale, eps=1e-2 * scale * scale)
    print(f"scale {scale}: worst fractions of the tolerances so far {worst}")


def test_derived_values_are_the_host_functions(ctx):
    h, w = 33, 129
    a, b = frames(h, w, np.uint8, np.float32)
    got, ref = ctx.image_metrics(a, b), reference(h, w, np.uint8, np.float32)
    for k in ("mse", "mse_r", "mse_g", "mse_b", "mae", "psnr", "relmse", "ssim"):
        assert got[k] == pytest.approx(ref[k], rel=1e-12), k
        assert got[k] == M.derive(got["sums"], 1.0, True)[k]
    print("129x33 u8 vs f32:", {k: got[k] for k in ("mse", "psnr", "mae", "max_abs", "relmse", "ssim")})
