"""GPU suite: what a workgroup does after its first tile, in kernels that deal tiles to a capped grid and stride over them.

The median's tiled kernel launches min(tiles, 4 x CU) workgroups of 64 x 16 tiles, the firefly clamp min(tiles, 8 x CU).  Frames here
are 192 texels wide -- three tile columns, the middle one with its whole halo inside the image at every radius -- and high enough for
2 cap + 3 tiles and two tile rows more, so some workgroups take three tiles, an interior one among them.  The cap is no multiple of 3 on the devices this runs on (asserted), so a
workgroup's successive tiles alternate between the border columns and the interior one: the median's vote for its plain selection
class (every texel of the tile and its halo inside the image and finite) flips between a workgroup's rounds.

Frames repeat a pattern of 37 rows (tests/tall_inputs.py), so every pixel is compared with the checker's output on a small frame.

    * median, plain class: radius 1, 2, 3 on a finite frame of sixteenths with many ties; every pixel against np_median and against
      the same frame with one all-zero layer (rank counting).  Then one NaN in an interior tile that is some workgroup's SECOND tile
      and one in an interior tile that is a workgroup's THIRD (the tiles from t % grid and t // grid; the frame is two tile rows higher
      than 2 cap + 3 tiles need, so that the third round holds interior tiles): outside the two windows the bits of the unplanted run,
      inside them the checker's values, every output finite.
    * median, weighted tiled class: 1 and 4 layers of integer levels at EXACT_SIGMA (weights exactly 0 or 1), bit for bit.
    * firefly clamp: bit for bit against np_firefly.
    * colour box (8 x CU): integer levels; at gamma 0 the checker's bits, at gamma > 0 the header's rule and the small frame's bits.
    * image metrics (4096): the map by its rule, the integer sums bit for bit, a second call into the uncleared workspace.
    * guided filter (at most 8192 workgroups over strips x 32-row segments): 3 x 524 800 at radius 1, 2 and 16 and 300 x 262 149 at
      radius 16, a float frame guiding itself and a uint8 frame with a uint8 guide, against np_guided under the header's bound.
"""
import ctypes

import numpy as np
import pytest
import torch

import firefly_inputs
import guided_inputs as gdi
import image_denoising_filter_amd as mid
import median_inputs as mi
import np_color_bounds
import np_firefly
import np_image_metrics as npm
import np_guided
import np_median
import tall_inputs as ti
from tall_device import F32F32, Plane, dev, finish, rows_on_device, table, wrong_rows

pytestmark = pytest.mark.gpu

W, TILES_X, TILE_H = 192, 3, 16


def geometry(per_cu):
    """(cap, h, tiles): the frame of 2 cap + 3 tiles or more; asserts that some workgroup takes three tiles."""
    cap = per_cu * torch.cuda.get_device_properties(0).multi_processor_count
    h = ti.later_tiles_height(cap, TILES_X, TILE_H) + 2 * TILE_H       # two tile rows more: the third round holds an interior tile
    tiles = TILES_X * ti.cdiv(h, TILE_H)
    grid = min(tiles, cap)
    assert tiles >= 2 * cap + 3 and grid == cap and ti.rounds_of(tiles, grid) >= 3
    print(f"cap {cap}: {W} x {h}, {tiles} tiles over {grid} workgroups, {ti.rounds_of(tiles, grid)} rounds")
    return cap, h, tiles


def interior(t, tiles):
    """Tile t lies in the middle column and in neither the first nor the last tile row: its halo is inside the image."""
    return t % TILES_X == 1 and 0 < t // TILES_X < tiles // TILES_X - 1


def median_192(ctx, frame, layers, h, radius):
    prm = mid.MedianParams(W, h, radius, F32F32 if layers else mid.FMT_RGBA32F)
    out = Plane((h, W, 4), torch.float32)
    L = len(layers)
    torch.cuda.synchronize()
    rc = mid.lib.mid_median_filter(ctx.handle, ctypes.byref(prm), (ctypes.c_float * 16)(*[mi.EXACT_SIGMA] * L) if L else None, frame.ptr,
                                   table(layers) if L else None, L, out.ptr, mid.FMT_RGBA32F, None)
    finish(ctx, rc, {"frame": frame, "layers": layers}, (out,))
    return out.mid


@pytest.mark.parametrize("radius", mi.RADII)
def test_median_plain_class_in_second_and_third_tiles(ctx, radius):
    cap, h, tiles = geometry(4)
    assert cap % TILES_X != 0, "the grid stride is a multiple of 3: a workgroup would stay in one tile column"
    # some workgroup goes border -> interior -> border, another interior -> border -> ...: the vote flips between rounds
    flips = [[interior(b + k * cap, tiles) for k in range(3) if b + k * cap < tiles] for b in range(cap)]
    assert [False, True, False] in flips and any(f[:2] == [True, False] for f in flips)
    second = next(b + cap for b in range(TILES_X, cap) if interior(b + cap, tiles))
    third = next(t for t in range(2 * cap, tiles) if interior(t, tiles))
    assert second // cap == 1 and third // cap == 2 and interior(second, tiles) and interior(third, tiles)
    assert second % cap != third % cap and any(len(f) == 3 and f[2] for f in flips), "some workgroup runs the plain class in its third tile"

    pattern = ti.tie_frame(ti.PERIOD, W)
    hs = ti.small_height(h, radius)
    want = np_median.median(ti.tile_rows(pattern, hs), None, None, radius)[0]
    frame = Plane((h, W, 4), torch.float32, pattern)
    rows = rows_on_device(h, radius, hs)
    plain = median_192(ctx, frame, [], h, radius)
    assert wrong_rows(plain, dev(want), rows) == [], "the plain class against the checker"
    zero = Plane((h, W, 4), torch.float32, np.zeros((ti.PERIOD, W, 4), np.float32))
    counted = median_192(ctx, frame, [zero], h, radius)
    assert torch.equal(plain.view(torch.int32), counted.view(torch.int32)), "the selection network against rank counting"
    del counted, zero

    spots = [((t // TILES_X) * TILE_H + 8, (t % TILES_X) * 64 + 32 + i) for i, t in enumerate((second, third))]
    for y, x in spots:
        frame.mid[y, x, 0] = float("nan")
    frame.before = int(frame.buf.sum(dtype=torch.int64))
    planted = median_192(ctx, frame, [], h, radius)
    assert bool(torch.isfinite(planted).all())
    differs = planted.view(torch.int32) != plain.view(torch.int32)
    for y, x in spots:
        crop = frame.mid[y - 8:y + 9].cpu().numpy()
        ref = np_median.median(crop, None, None, radius)[0]
        win = (slice(8 - radius, 9 + radius), slice(x - radius, x + radius + 1))
        got = planted[y - 8:y + 9].cpu().numpy()
        assert np_median.same_values(got[win], ref[win]).all(), "inside a planted window: the checker's values"
        differs[y - radius:y + radius + 1, x - radius:x + radius + 1] = False
    assert not bool(differs.any()), "outside the planted windows: the bits of the unplanted run"


@pytest.mark.parametrize("n_layers", (1, 4))
@pytest.mark.parametrize("radius", mi.RADII)
def test_median_weighted_tiled_class_in_later_tiles(ctx, radius, n_layers):
    cap, h, tiles = geometry(4)
    pattern = ti.tie_frame(ti.PERIOD, W)
    guide = mi.exact_scene(ti.PERIOD, W, seed=3)[1]
    layers = [guide * np.float32(l + 1) for l in range(n_layers)]
    hs = ti.small_height(h, radius)
    want, _, exact = np_median.median(ti.tile_rows(pattern, hs), [ti.tile_rows(l, hs) for l in layers], [mi.EXACT_SIGMA] * n_layers, radius)
    assert exact.all()
    frame = Plane((h, W, 4), torch.float32, pattern)
    got = median_192(ctx, frame, [Plane((h, W, 4), torch.float32, l) for l in layers], h, radius)
    assert wrong_rows(got, dev(want), rows_on_device(h, radius, hs)) == []


@pytest.mark.parametrize("radius,rank", ((1, 1), (2, 3)))
def test_firefly_clamp_in_later_tiles(ctx, radius, rank):
    cap, h, tiles = geometry(8)
    pattern = firefly_inputs.frame_of((ti.PERIOD, W), np.float32, seed=1)
    hs = ti.small_height(h, radius)
    want = np_firefly.firefly_clamp(ti.tile_rows(pattern, hs), radius, rank)
    frame = Plane((h, W, 4), torch.float32, pattern)
    out = Plane((h, W, 4), torch.float32)
    prm = mid.FireflyParams(W, h, radius, rank, 1.0, 0.0, mid.FMT_RGBA32F)
    torch.cuda.synchronize()
    rc = mid.lib.mid_firefly_clamp(ctx.handle, ctypes.byref(prm), frame.ptr, out.ptr, None)
    finish(ctx, rc, {"frame": frame}, (out,))
    assert bool(torch.isfinite(out.mid).all())
    assert wrong_rows(out.mid, dev(want), rows_on_device(h, radius, hs)) == []


# ---- the guided filter: at most 8192 workgroups stride over strips x segments of 32 rows, vertical running sums in registers ------------
GUIDED_CAP = 8192
FMT = {np.dtype(np.float32): mid.FMT_RGBA32F, np.dtype(np.uint8): mid.FMT_RGBA8}


def guided(ctx, frame, guide, h, w, radius):
    fdt = np.dtype(np.float32 if frame.dtype == torch.float32 else np.uint8)
    gdt = fdt if guide is None else np.dtype(np.float32 if guide.dtype == torch.float32 else np.uint8)
    prm = mid.GuidedParams(w, h, radius, gdi.EPS, mid.api.fmt_with_guide(FMT[fdt], FMT[gdt]))
    n = ctypes.c_size_t()
    assert mid.lib.mid_guided_workspace(ctypes.byref(prm), ctypes.byref(n)) == 0
    work, out = Plane((n.value,), torch.uint8), Plane((h, w, 4), torch.float32)
    torch.cuda.synchronize()
    rc = mid.lib.mid_guided_filter(ctx.handle, ctypes.byref(prm), frame.ptr, None if guide is None else guide.ptr, work.ptr, out.ptr, mid.FMT_RGBA32F, None)
    finish(ctx, rc, {"frame": frame, "guide": [] if guide is None else [guide]}, (work, out))
    return out.mid


@pytest.mark.parametrize("kind", ("self-f32", "guide-u8"))
@pytest.mark.parametrize("shape", ((524800, 3, 1), (524800, 3, 2), (524800, 3, 16), (262149, 300, 16)), ids=lambda s: f"{s[1]}x{s[0]}-r{s[2]}")
def test_guided_filter_in_later_segments(ctx, shape, kind):
    """The kernel's running sums depend on a row's place in its 32-row segment, and 37 and 32 are coprime: the tall output is held to
    the float64 checker of the small frame under the header's bound, |out - exact| <= 8 * 2^-24 * T, not to GPU bits."""
    h, w, radius = shape
    segments = ti.cdiv(h, gdi.PERIOD) * ti.cdiv(w, gdi.strip_w(radius))
    assert segments > 2 * GUIDED_CAP, "some workgroup takes a third segment"
    noisy, alb, _ = gdi.scene(ti.PERIOD, w, radius)
    fpat, gpat = (noisy, None) if kind == "self-f32" else (gdi.as_dtype(noisy, np.uint8), gdi.as_dtype(alb, np.uint8))
    reach = 2 * radius                                      # the box of the coefficients over the box of the moments
    hs = ti.small_height(h, reach)
    ref = np_guided.guided(ti.tile_rows(fpat, hs), None if gpat is None else ti.tile_rows(gpat, hs), radius, gdi.EPS)
    assert ref["filtered"].all()
    tdt = torch.float32 if fpat.dtype == np.float32 else torch.uint8
    frame = Plane((h, w, 4), tdt, fpat)
    guide = None if gpat is None else Plane((h, w, 4), tdt, gpat)
    got = guided(ctx, frame, guide, h, w, radius)
    assert bool(torch.isfinite(got).all()), "a pixel was not written"
    rows = rows_on_device(h, reach, hs)
    assert torch.equal(got[..., 3].double(), dev(ref["out"][..., 3]).index_select(0, rows)), "alpha is the frame's"
    err = (got[..., :3].double() - dev(ref["out"][..., :3]).index_select(0, rows)).abs_()
    share = float((err / dev(np_guided.tolerance(ref)).index_select(0, rows)).max())
    print(f"guided {w} x {h} radius {radius} {kind}: {segments} segments over {GUIDED_CAP} workgroups, worst share of the bound {share:.3f}")
    assert share <= 1.0


# ---- the colour box: min(tiles, 8 x CU) workgroups over 64 x 16 tiles ---------------------------------------------------------------------
def color_bounds(ctx, frame, h, radius, gamma):
    lo, hi = Plane((h, W, 4), torch.float32), Plane((h, W, 4), torch.float32)
    prm = mid.ColorBoundsParams(W, h, radius, gamma, mid.FMT_RGBA32F)
    torch.cuda.synchronize()
    rc = mid.lib.mid_color_bounds(ctx.handle, ctypes.byref(prm), frame.ptr, lo.ptr, hi.ptr, None)
    finish(ctx, rc, {"frame": frame}, (lo, hi))
    return lo.mid, hi.mid


@pytest.mark.parametrize("radius,gamma", ((1, 0.0), (2, 0.0), (1, 1.0), (2, 2.5)))
def test_color_bounds_in_later_tiles(ctx, radius, gamma):
    """Frames of integer levels 0 .. 255 with a NaN, a +Inf and a -Inf texel per period.  The window sums of such a frame are exact,
    so the mean -- which the contract rounds to float32 -- and the count have the checker's bits: at gamma = 0, where lo = hi = mu,
    every pixel is held to np_color_bounds bit for bit.  With gamma > 0 the contract's deviation is a float64 square root that no
    fp32 kernel reproduces to the bit (the header gives 1e-5 max(1, |mu| + gamma sigma) for it): there the tall frame is held to the
    checker by that rule, .w and the infinities exactly, and bit for bit to the GPU's own small frame -- the kernel sums a pixel's
    window in one order wherever the pixel lies in its tile."""
    cap, h, tiles = geometry(8)
    rng = np.random.default_rng(12)
    pattern = rng.integers(0, 256, (ti.PERIOD, W, 4)).astype(np.float32)
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        pattern[5 + 11 * k, 70 + 3 * k, k] = bad
    assert ti.distinct_rows(pattern)
    hs = ti.small_height(h, radius)
    sc = {}
    with np.errstate(invalid="ignore", over="ignore"):
        ref = np_color_bounds.color_bounds(ti.tile_rows(pattern, hs), radius, gamma, scale=sc)
    small = color_bounds(ctx, Plane((hs, W, 4), torch.float32, pattern), hs, radius, gamma)
    got = color_bounds(ctx, Plane((h, W, 4), torch.float32, pattern), h, radius, gamma)
    rows = rows_on_device(h, radius, hs)
    for name, g, sm, r in zip(("lo", "hi"), got, small, ref):
        assert not torch.isnan(g).any(), f"{name}: a pixel was not written"
        r32 = dev(r.astype(np.float32))
        if gamma == 0.0:
            assert wrong_rows(g, r32, rows) == [], f"{name}: the checker's bits"
            continue
        assert wrong_rows(g, sm, rows) == [], f"{name}: the bits of the GPU's own small frame"
        want = dev(r).index_select(0, rows)
        assert torch.equal(g[..., 3].double(), want[..., 3]), f"{name}: the validity count"
        inf = torch.isinf(want[..., :3])
        assert torch.equal(g[..., :3].double()[inf], want[..., :3][inf]), f"{name}: n == 0"
        scale = dev(sc["scale"]).index_select(0, rows).clamp(min=1.0)
        err = ((g[..., :3].double() - want[..., :3]).abs() / scale)[~inf]
        print(f"color_bounds {name} radius {radius} gamma {gamma}: {float(err.max()):.2e} of max(1, |mu| + gamma sigma)")
        assert float(err.max()) <= 1e-5


# ---- the image metrics: at most 4096 workgroups over 64 x 16 tiles, partial sums in a workspace --------------------------------------------
METRICS_CAP, METRICS_PEAK, METRICS_EPS, METRICS_REACH = 4096, 16.0, 1e-2, npm.R


def image_metrics(ctx, a, b, work, h):
    """One call into `work` (not cleared here); returns (the 16 sums as float64 numpy, the map on the device)."""
    out = Plane((h, W), torch.float32)
    prm = mid.ImageMetricsParams(W, h, mid.FMT_RGBA32F, mid.FMT_RGBA32F, METRICS_PEAK, METRICS_EPS, 1)
    torch.cuda.synchronize()
    rc = mid.lib.mid_image_metrics(ctx.handle, ctypes.byref(prm), a.ptr, b.ptr, work.ptr, out.ptr, None)
    finish(ctx, rc, {"a": a, "b": b}, (work, out))
    return work.mid[:8 * mid.METRICS_N].view(torch.float64).cpu().numpy().copy(), out.mid


def test_image_metrics_in_later_tiles(ctx):
    """Frames of integer levels 0 .. 15: the counts, the squared and absolute sums and the largest difference are integers, exact in
    binary64 in any order, so they are held bit for bit to the checker's sums of one period times the number of periods plus those of
    the remaining rows.  relMSE's sums (a quotient per term) and the SSIM mean keep the header's tolerances, the map its rule per
    pixel through the period.  A second call into the same, uncleared workspace gives the first call's bits."""
    h = ti.later_tiles_height(METRICS_CAP, TILES_X, TILE_H)
    tiles = TILES_X * ti.cdiv(h, TILE_H)
    assert tiles >= 2 * METRICS_CAP + 3 and ti.rounds_of(tiles, METRICS_CAP) >= 3
    print(f"cap {METRICS_CAP}: {W} x {h}, {tiles} tiles, {ti.rounds_of(tiles, METRICS_CAP)} rounds")
    rng = np.random.default_rng(13)
    pa = rng.integers(0, 16, (ti.PERIOD, W, 4)).astype(np.float32)
    pb = np.clip(pa + rng.integers(-2, 3, pa.shape), 0, 15).astype(np.float32)
    pa[9, 100, 1] = np.nan
    assert ti.distinct_rows(pa) and ti.distinct_rows(pb)
    kw = dict(peak=METRICS_PEAK, eps=METRICS_EPS)
    whole, rest = h // ti.PERIOD, h % ti.PERIOD
    per, rem = npm.image_metrics(pa, pb, ssim=False, **kw)["sums"], npm.image_metrics(pa[:rest], pb[:rest], ssim=False, **kw)["sums"]
    hs = ti.small_height(h, METRICS_REACH)
    ref = npm.image_metrics(ti.tile_rows(pa, hs), ti.tile_rows(pb, hs), **kw)
    a, b = Plane((h, W, 4), torch.float32, pa), Plane((h, W, 4), torch.float32, pb)
    n_work = mid.lib.mid_image_metrics_workspace(W, h)
    work = Plane((n_work,), torch.uint8)
    sums, got = image_metrics(ctx, a, b, work, h)
    again, got2 = image_metrics(ctx, a, b, work, h)
    assert np.array_equal(sums.view(np.uint64), again.view(np.uint64)), "a second call into the uncleared workspace"
    assert torch.equal(got.view(torch.int32), got2.view(torch.int32))
    n = whole * per[npm.I_VALID] + rem[npm.I_VALID]
    for i in (npm.I_VALID, npm.I_INVALID, *range(npm.I_SQ, npm.I_SQ + 3), *range(npm.I_ABS, npm.I_ABS + 3)):
        assert sums[i] == whole * per[i] + rem[i], (i, sums[i], whole * per[i] + rem[i])
    assert sums[npm.I_MAX] == max(per[npm.I_MAX], rem[npm.I_MAX]) and sums[npm.I_INVALID] == h * W - n > 0
    for i in range(npm.I_REL, npm.I_REL + 3):
        want = whole * per[i] + rem[i]
        assert abs(sums[i] - want) <= npm.sum_rtol(n) * want, (i, sums[i], want)
    rows_np = ti.row_map(h, METRICS_REACH, hs)
    valid = ref["valid"]
    mean = float(np.bincount(rows_np, minlength=hs) @ np.where(valid, ref["map"], 0.0).sum(1)) / n
    tol = float(npm.ssim_atol(ref["M"].max(), METRICS_PEAK))
    print(f"ssim mean {sums[npm.I_SSIM] / n:.12f} against {mean:.12f}: {abs(sums[npm.I_SSIM] / n - mean) / tol:.3f} of its tolerance")
    assert abs(sums[npm.I_SSIM] / n - mean) <= tol
    rows = rows_on_device(h, METRICS_REACH, hs)
    assert torch.equal(torch.isnan(got), dev(~valid).index_select(0, rows)), "NaN exactly where the pixel is not valid"
    rmap = np.where(valid, ref["map"], 0.0)
    rtol = np.where(valid, npm.ssim_atol(ref["M"], METRICS_PEAK) + np.abs(rmap) * 2.0 ** -24, 1.0)
    share = (torch.nan_to_num(got).double() - dev(rmap).index_select(0, rows)).abs() / dev(rtol).index_select(0, rows)
    print(f"ssim map: worst {float(share.max()):.3f} of its tolerance")
    assert float(share.max()) <= 1.0
