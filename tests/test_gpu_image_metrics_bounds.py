"""GPU suite: what mid_image_metrics (section a4n) touches and what it refuses.

Guard bands of 64 rows behind `work` (at exactly the size the workspace query returns) and behind `map`, NaN bytes around both inputs;
NaN / +-Inf texels planted in a, in b and in both on corners, edges and tile seams; a frame with nothing valid; a 262149 x 1 strip and
a 1 x 70000 column (more tiles than workgroups); and every refusal, with `work` and `map` untouched."""
import ctypes

import numpy as np
import pytest
import torch

import image_denoising_filter_amd as mid
import np_image_metrics as M
from image_metrics_inputs import pair
from test_gpu_image_metrics import holds

pytestmark = pytest.mark.gpu
FMT = {np.dtype(np.float32): mid.FMT_RGBA32F, np.dtype(np.uint8): mid.FMT_RGBA8, np.dtype(np.float16): mid.FMT_RGBA16F}
GUARD = 0xA5


def guarded_input(x):
    """x on the device inside a buffer whose every other byte is 0xFF (NaN as a float or a half), 4 KiB on either side."""
    raw = torch.full((x.nbytes + 8192,), 0xFF, dtype=torch.uint8, device="cuda:0")
    raw[4096:4096 + x.nbytes] = torch.from_numpy(x.view(np.uint8).reshape(-1)).to("cuda:0")
    return raw, raw.data_ptr() + 4096


def call(ctx, a, b, peak=1.0, eps=1e-2, ssim=1, want_map=True):
    """The C entry point on guarded buffers: (sums, map or None); asserts that the guards and the inputs' surroundings are intact."""
    h, w = a.shape[:2]
    nw = mid.lib.mid_image_metrics_workspace(w, h)
    assert nw == 128 * (1 + min(4096, -(-w // 64) * -(-h // 16)))
    band_w, band_m = 64 * 128, 64 * w * 4
    work = torch.full((nw + band_w,), GUARD, dtype=torch.uint8, device="cuda:0")
    smap = torch.full((h * w * 4 + band_m,), GUARD, dtype=torch.uint8, device="cuda:0")
    ra, pa = guarded_input(a)
    rb, pb = guarded_input(b)
    p = mid.ImageMetricsParams(w, h, FMT[a.dtype], FMT[b.dtype], peak, eps, ssim)
    torch.cuda.synchronize()
    rc = mid.lib.mid_image_metrics(ctx.handle, ctypes.byref(p), pa, pb, work.data_ptr(), smap.data_ptr() if want_map else None, None)
    assert rc == 0, mid.lib.mid_last_error()
    ctx.sync()
    assert bool((work[nw:] == GUARD).all()), "the band behind work"
    assert bool((smap[h * w * 4:] == GUARD).all()), "the band behind map"
    if not want_map:
        assert bool((smap == GUARD).all())
    for raw, x in ((ra, a), (rb, b)):
        assert bool((raw[:4096] == 0xFF).all()) and bool((raw[4096 + x.nbytes:] == 0xFF).all())
        assert np.array_equal(raw[4096:4096 + x.nbytes].cpu().numpy(), x.view(np.uint8).reshape(-1))
    sums = work[:128].cpu().numpy().view(np.float64).copy()
    m = smap[:h * w * 4].cpu().numpy().view(np.float32).reshape(h, w).copy() if want_map else None
    return sums, m


def as_result(sums, m, peak=1.0, ssim=True):
    r = mid.metrics_derive(sums, peak, ssim)
    r["sums"] = sums
    if m is not None:
        r["map"] = m
    return r


@pytest.mark.parametrize("shape", [(1, 1), (5, 5), (17, 65), (33, 129)], ids=lambda s: f"{s[1]}x{s[0]}")
@pytest.mark.parametrize("dts", [(np.float32, np.float32), (np.uint8, np.float16)], ids=["f32-f32", "u8-f16"])
def test_guard_bands(ctx, shape, dts):
    h, w = shape
    a, b = pair(h, w)
    a = np.clip(np.rint(a * 255), 0, 255).astype(np.uint8) if dts[0] == np.uint8 else a.astype(dts[0])
    b = b.astype(dts[1])
    ref = M.image_metrics(a, b)
    sums, m = call(ctx, a, b)
    holds(as_result(sums, m), ref, 1.0, True, True)
    sums2, _ = call(ctx, a, b, want_map=False)
    sums0, _ = call(ctx, a, b, ssim=0, want_map=False)
    assert sums2.tobytes() == sums.tobytes() and sums0[:12].tobytes() == sums[:12].tobytes() and sums0[12] == 0


def plant(h, w, seed):
    """NaN / +-Inf in a, in b and in both: the four corners, the edges, both sides of the tile seams at x = 64 and y = 16."""
    a, b = pair(h, w)
    rng = np.random.default_rng(seed)
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0), (h - 1, w // 3), (h // 3, w - 1)]
    spots += [(y, x) for y in (15, 16) for x in (63, 64) if y < h and x < w] + [(min(h - 1, 21), min(w - 1, 69)), (min(h - 1, 10), min(w - 1, 5))]
    spots = sorted(set(spots))
    for k, (y, x) in enumerate(spots):
        bad, c = (np.nan, np.inf, -np.inf)[k % 3], int(rng.integers(3))
        if k % 3 != 1:
            a[y, x, c] = bad
        if k % 3 != 0:
            b[y, x, (c + 1) % 3] = bad
    a[h // 2, w // 2, 3] = np.nan                                                # a non-finite ALPHA does not count
    return a, b, spots


@pytest.mark.parametrize("shape", [(2, 2), (17, 65), (33, 129), (40, 200)], ids=lambda s: f"{s[1]}x{s[0]}")
@pytest.mark.parametrize("dt", [np.float32, np.float16], ids=["f32", "f16"])
def test_non_finite_texels(ctx, shape, dt):
    h, w = shape
    a, b, spots = plant(h, w, h + w)
    a, b = a.astype(dt), b.astype(dt)
    ref = M.image_metrics(a, b)
    assert ref["n_invalid"] == len(spots) and ref["n_valid"] == h * w - len(spots)
    sums, m = call(ctx, a, b)
    assert sums[M.I_VALID] == h * w - len(spots) and sums[M.I_INVALID] == len(spots)
    bad = np.zeros((h, w), bool)
    for y, x in spots:
        bad[y, x] = True
    assert np.array_equal(np.isnan(m), bad)                                     # the map's NaN sits exactly there
    holds(as_result(sums, m), ref, 1.0, True, True)
    assert np.isfinite(sums).all()


def test_nothing_valid(ctx):
    h, w = 19, 70
    a, b = pair(h, w)
    a[..., 1] = np.nan
    sums, m = call(ctx, a, b)
    assert sums[M.I_VALID] == 0 and sums[M.I_INVALID] == h * w and sums[2:].tobytes() == np.zeros(14).tobytes()
    assert np.isnan(m).all()
    r = mid.metrics_derive(sums)
    assert all(np.isnan(r[k]) for k in ("mse", "mse_r", "mse_g", "mse_b", "mae", "psnr", "relmse", "ssim")) and r["max_abs"] == 0


@pytest.mark.parametrize("shape", [(1, 262149), (70000, 1)], ids=["262149x1", "1x70000"])
def test_more_tiles_than_workgroups(ctx, shape):
    h, w = shape
    n = h * w
    rng = np.random.default_rng(n)
    b = np.ones((h, w, 4), np.float32)
    b[..., :3] = (rng.integers(0, 64, (h, w, 3)) / 64.0).astype(np.float32)
    a = b.copy()
    flat_a = a.reshape(n, 4)
    where = np.unique(np.minimum([0, 1, 63, 64, 4095 * 16, 4096 * 16, 4096 * 64, n // 2, n - 2, n - 1], n - 1))    # both sides of tile and workgroup seams
    assert n // 3 not in where
    flat_a[where, 0] += np.float32(0.25)
    flat_a[n // 3, 2] = np.nan
    ref = M.image_metrics(a, b)
    sums, m = call(ctx, a, b)
    assert sums[M.I_VALID] == n - 1 and sums[M.I_INVALID] == 1
    assert sums[M.I_SQ] == len(where) / 16.0 and sums[M.I_ABS] == len(where) / 4.0 and sums[M.I_MAX] == 0.25      # exact: sixteenths
    assert sums[M.I_SQ + 1] == 0 and sums[M.I_SQ + 2] == 0
    holds(as_result(sums, m), ref, 1.0, True, True)


def test_refusals_leave_the_outputs_untouched(ctx):
    h, w = 20, 70
    a, b = pair(h, w)
    da, db = ctx.upload(a), ctx.upload(b)
    nw = mid.lib.mid_image_metrics_workspace(w, h)
    work = torch.full((nw + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    smap = torch.full((h * w * 4 + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    both = torch.full((nw + h * w * 4,), GUARD, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    W, Mp = work.data_ptr(), smap.data_ptr()
    assert W % 16 == 0 and Mp % 16 == 0
    F = mid.FMT_RGBA32F
    good = dict(width=w, height=h, format_a=F, format_b=F, peak=1.0, eps=1e-2, ssim=1)

    def refused(word, ctx_h=ctx.handle, params=True, a=da.ptr, b=db.ptr, work=W, smap=Mp, **kw):
        p = mid.ImageMetricsParams(**{**good, **kw})
        rc = mid.lib.mid_image_metrics(ctx_h, ctypes.byref(p) if params else None, a, b, work, smap, None)
        assert rc == 1, (word, kw, rc)                                          # MID_ERR_INVALID
        msg = mid.lib.mid_last_error().decode()
        assert word in msg, (word, msg)

    refused("context is NULL", ctx_h=None)
    refused("params is NULL", params=False)
    refused("NULL pointer", a=None)
    refused("NULL pointer", b=None)
    refused("NULL pointer", work=None)
    for kw in (dict(width=0), dict(height=0), dict(width=-3)):
        refused("bad size", **kw)
    refused("too large", width=1 << 15, height=1 << 15)
    refused("unknown format_a", format_a=3)
    refused("unknown format_b", format_b=7)
    refused("unknown format_a", format_a=1 << 16)
    refused("guide bits", format_a=mid.api.fmt_with_guide(F, mid.FMT_RGBA8))
    refused("guide bits", format_b=mid.api.fmt_with_guide(mid.FMT_RGBA8, mid.FMT_RGBA16F))
    refused("a is not 16-byte aligned", a=da.ptr + 8)
    refused("b is not 16-byte aligned", b=db.ptr + 4)
    refused("a is not 8-byte aligned", a=da.ptr + 4, format_a=mid.FMT_RGBA16F)
    refused("b is not 4-byte aligned", b=db.ptr + 2, format_b=mid.FMT_RGBA8)
    refused("work is not 16-byte aligned", work=W + 8)
    refused("map is not 4-byte aligned", smap=Mp + 2)
    for v in (0.0, -1.0, float("nan"), float("inf")):
        refused("peak", peak=v)
        refused("eps", eps=v)
    for v in (-1, 2):
        refused("ssim", ssim=v)
    refused("a map needs ssim == 1", ssim=0)
    refused("work overlaps an input", work=da.ptr)
    refused("work overlaps an input", work=db.ptr + 16 * (h * w - 1))
    refused("map overlaps an input", smap=da.ptr + 4 * 5)
    refused("map overlaps an input", smap=db.ptr)
    refused("map overlaps work", work=both.data_ptr(), smap=both.data_ptr() + nw - 4)
    refused("map overlaps work", work=both.data_ptr() + h * w * 4 - 16 - (h * w * 4 - 16) % 16, smap=both.data_ptr())
    ctx.sync()
    torch.cuda.synchronize()
    for buf in (work, smap, both):
        assert bool((buf == GUARD).all())
    assert np.array_equal(ctx.download(da, a.shape, np.float32), a) and np.array_equal(ctx.download(db, b.shape, np.float32), b)
    # and what is allowed: a == b, ssim == 0 without a map, the map right behind the workspace
    p = mid.ImageMetricsParams(**good)
    assert mid.lib.mid_image_metrics(ctx.handle, ctypes.byref(p), da.ptr, da.ptr, both.data_ptr(), both.data_ptr() + nw, None) == 0, mid.lib.mid_last_error()
    ctx.sync()
    assert both[:128].cpu().numpy().view(np.float64)[M.I_SSIM] == h * w
