"""Layer-guided NLM (mid_nlm_layers_accum, mid_nlm_layers, mid_nlm_layers_pair_accum, mid_nlm_layers_temporal) where kernels go
wrong unnoticed: frames smaller than a tile, a wave or the search window; frames that end exactly at, or one past, a tile seam of
the strip kernels (64 rows x 58 columns for the 21x21 / 7x7 window, 64 x 59 for the 14x14 / 6x6 one); every tile count from 1 to 17
and a few larger grids (the XCD remap of the tile index); HDR magnitudes and the range of the filtering parameter; NaN and +-Inf
texels; and the guide's alpha byte, which the contract does not read.  Every comparison is with the float64 checkers
(np_nlm_layers, np_nlm_layers_temporal; tests/test_nlm_layers_checker_edges.py anchors them at these shapes) at the NLM parity
tolerance, and the fused calls against their chains of dispatches bit for bit."""
import ctypes

import numpy as np
import pytest

import image_denoising_filter_amd as mid
import np_nlm_layers
import np_nlm_layers_temporal as chk
from conftest import rel_err, synth_hdr
from test_gpu_nlm_layers import H, NLM_CFGS, TOL, bits, guides, noisy
from test_gpu_nlm_layers_temporal import chain, sequence

# (the checkers share the search offsets out over threads, and NumPy's error state is per thread: np.errstate does not reach them)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")]

STRIP = ("ref", "bench")                    # the two LDS-tiled strip kernels
PER_PIXEL = ("generic", "rt16", "naive")    # the per-pixel kernel: 3x3, the 16-wide and the lopsided patch
VW = {"ref": 59, "bench": 58}               # output columns of a strip-kernel tile: 64 - (patch width - 1)
TILE_H = 64

TINY = [(1, 1), (1, 40), (40, 1), (2, 70), (70, 2), (9, 9), (3, 5)]
SEAMS = [(63, 57), (64, 58), (64, 59), (65, 59), (65, 60), (128, 116), (128, 118), (129, 117), (129, 119)]


def sums_plus(W, num, den):
    """The five used floats of WeightInfo after a dispatch with the checker's sums (num, den) into W."""
    want = W[..., :5].astype(np.float64)
    want[..., :4] += num
    want[..., 4] += den
    return want


# ---- a. tiny and ragged frames ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", STRIP + PER_PIXEL)
@pytest.mark.parametrize("shape", TINY + SEAMS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny_and_ragged_frames(ctx, cfg, shape):
    h, w = shape
    win = NLM_CFGS[cfg]
    translucent = (TINY + SEAMS).index(shape) % 2 == 1      # alpha 0.5 in 3 % of the texels: the non-opaque form of the weight sums
    rng = np.random.default_rng(1000 * h + w + len(cfg))
    img = noisy(rng, h, w, translucent)
    gl = guides(rng, h, w, 3)
    worst = 0.0
    # the fused call against the checker, and against its chain of accumulate dispatches + normalize
    for L in (1, 3):
        got = ctx.nlm_layers(img, gl[:L], H, **win)
        e = rel_err(got, np_nlm_layers.nlm_layers(img, gl[:L], H, **win))
        worst = max(worst, e)
        assert e < TOL, (cfg, shape, L, e)
    W = np.zeros((h, w, 8), np.float32)
    for g in gl:
        W = ctx.nlm_layers_accum(img, g, W, H, **win)
    assert np.array_equal(bits(got), bits(ctx.normalize(W))), (cfg, shape)
    # one accumulate dispatch into a non-zero W: the five used floats, and the three pad floats untouched
    W = (rng.random((h, w, 8)) + 0.5).astype(np.float32)
    Wg = ctx.nlm_layers_accum(img, gl[0], W, H, **win)
    e = rel_err(Wg[..., :5], sums_plus(W, *np_nlm_layers.nlm_layers_sums(img, gl[:1], H, **win)))
    worst = max(worst, e)
    assert e < TOL, (cfg, shape, "accumulate", e)
    assert np.array_equal(bits(Wg[..., 5:]), bits(W[..., 5:])), (cfg, shape, "pad floats")
    # over neighbouring frames
    frames, layers = sequence(rng, h, w, 3, 2, translucent)
    got = ctx.nlm_layers_temporal(frames, layers, 1, hparam=H, **win)
    want = chk.nlm_layers_temporal(frames, layers, 1, H, **win)
    for t in range(3):
        e = rel_err(got[t], want[t])
        worst = max(worst, e)
        assert e < TOL, (cfg, shape, "temporal", t, e)
        assert np.array_equal(bits(got[t]), bits(chain(ctx, frames, layers, 1, t, win))), (cfg, shape, t)
    print(f"{cfg} {h}x{w}: worst rel err {worst:.2e}")


@pytest.mark.parametrize("cfg", STRIP + ("generic",))
@pytest.mark.parametrize("shape", TINY + SEAMS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nothing_is_written_beyond_the_frame(ctx, cfg, shape):
    # The last tile row of a strip kernel has rows at and below the frame's end (whole waves of 8 rows, and the tail of the wave that
    # holds row h - 1), its last tile column has lanes right of it; a write from one of them lands in the next row or behind the
    # buffer, where no comparison of the h x w result sees it.  So the output and W get GUARD more rows of random bits -- a whole
    # tile's height -- which every entry point must leave alone, while the frame's own rows keep the bits of the plain call.
    GUARD = TILE_H
    h, w = shape
    win = NLM_CFGS[cfg]
    rng = np.random.default_rng(3000 * h + w + len(cfg))
    frames, layers = sequence(rng, h, w, 2, 2, translucent=True)
    p = ctypes.byref(mid.NlmParams(w, h, H, *win["search"], *win["patch"], mid.FMT_RGBA32F))
    d_fr = [ctx.upload(f) for f in frames]
    d_l = [[ctx.upload(g) for g in ls] for ls in layers]

    def guarded(depth, call, want):
        host = (rng.random((h + GUARD, w, depth)) + 0.5).astype(np.float32)
        d = ctx.upload(host)
        assert call(d.ptr) == 0, mid.lib.mid_last_error()
        ctx.sync()
        got = ctx.download(d, host.shape, np.float32)
        assert np.array_equal(bits(got[:h]), bits(want(host[:h]))), (cfg, shape, "the frame's rows")
        assert np.array_equal(bits(got[h:]), bits(host[h:])), (cfg, shape, "rows beyond the frame")

    tbl = (ctypes.c_void_p * 2)(*[d.ptr for d in d_l[0]])
    guarded(4, lambda o: mid.lib.mid_nlm_layers(ctx.handle, p, d_fr[0].ptr, tbl, 2, o, None),
            lambda _: ctx.nlm_layers(frames[0], layers[0], H, **win))
    guarded(8, lambda o: mid.lib.mid_nlm_layers_accum(ctx.handle, p, d_fr[0].ptr, d_l[0][1].ptr, o, None),
            lambda W: ctx.nlm_layers_accum(frames[0], layers[0][1], W, H, **win))
    guarded(8, lambda o: mid.lib.mid_nlm_layers_pair_accum(ctx.handle, p, d_l[0][0].ptr, d_l[1][0].ptr, d_fr[1].ptr, o, None),
            lambda W: ctx.nlm_layers_pair_accum(layers[0][0], layers[1][0], frames[1], W, H, **win))
    fr = (ctypes.c_void_p * 2)(*[d.ptr for d in d_fr])
    ly = (ctypes.c_void_p * 4)(*[d.ptr for ls in d_l for d in ls])
    guarded(4, lambda o: mid.lib.mid_nlm_layers_temporal(ctx.handle, p, fr, ly, 2, 2, 1, 1, 1, (ctypes.c_void_p * 1)(o), mid.FMT_RGBA32F, None),
            lambda _: ctx.nlm_layers_temporal(frames, layers, 1, 1, 1, hparam=H, **win)[0])


# ---- b. every tile count ---------------------------------------------------------------------------------------------------------
def _tile_cases():
    out = []
    for cfg in STRIP:
        for T in range(1, 18):                                          # a row of T tiles, a column of T tiles
            out += [(cfg, TILE_H, VW[cfg] * T), (cfg, TILE_H * T, VW[cfg])]
        for ty, tx in ((4, 6), (5, 5), (7, 9), (8, 8), (5, 13)):        # 24, 25, 63, 64, 65 tiles, the last row and column ragged
            out.append((cfg, TILE_H * ty - 3, VW[cfg] * tx - 5))
    return sorted(set(out))


@pytest.mark.parametrize("cfg,h,w", _tile_cases(), ids=lambda v: str(v))
def test_every_tile_count(ctx, cfg, h, w):
    # a tile the remap leaves out keeps W's old value (accumulate) or the output buffer's old bytes (fused); a tile dealt twice is
    # added twice to W.  Every pixel is compared, with fresh random data per case.
    win = NLM_CFGS[cfg]
    tiles = -(-h // TILE_H) * -(-w // VW[cfg])
    rng = np.random.default_rng(7919 * h + w)
    frames, layers = sequence(rng, h, w, 2, 2)
    s = [np_nlm_layers.nlm_layers_sums(frames[0], [g], H, **win) for g in layers[0]]      # the dispatches (0, 0, l)
    W = (rng.random((h, w, 8)) + 0.5).astype(np.float32)
    e_acc = rel_err(ctx.nlm_layers_accum(frames[0], layers[0][0], W, H, **win)[..., :5], sums_plus(W, *s[0]))
    e_fused = rel_err(ctx.nlm_layers(frames[0], layers[0], H, **win), chk.normalize(s[0][0] + s[1][0], s[0][1] + s[1][1]))
    want = chk.nlm_layers_temporal(frames, layers, 1, H, **win, first=0, count=1, cache={(0, 0, 0): s[0], (0, 0, 1): s[1]})[0]
    e_temp = rel_err(ctx.nlm_layers_temporal(frames, layers, 1, 0, 1, hparam=H, **win)[0], want)
    print(f"{cfg} {h}x{w} ({tiles} tiles): accumulate {e_acc:.2e} fused {e_fused:.2e} temporal {e_temp:.2e}")
    assert e_acc < TOL and e_fused < TOL and e_temp < TOL, (cfg, h, w, tiles)


# ---- c. HDR colours and the range of h -------------------------------------------------------------------------------------------
def _hdr(rng, h, w):
    """conftest.synth_hdr with its peak at 6e4: inside binary16, and 441 weights of 1 stay far below fp32 overflow."""
    img = synth_hdr(rng, h, w)
    img[..., :3] *= np.float32(6.0e4) / img[..., :3].max()
    return img.astype(np.float16).astype(np.float32)       # (so that the float16 frames below ARE these frames)


@pytest.mark.parametrize("cfg", STRIP + ("generic",))
@pytest.mark.parametrize("hp", [0.02, 0.1, 0.5, 2.0, 50.0])
def test_hdr_range_and_h_sweep(ctx, cfg, hp):
    rng = np.random.default_rng(31)
    h, w = 70, 150
    win = NLM_CFGS[cfg]
    _, layers = sequence(rng, h, w, 2, 2)
    frames = [_hdr(rng, h, w) for _ in range(2)]
    assert 5.9e4 < max(f.max() for f in frames) < 65504
    got = ctx.nlm_layers(frames[0], layers[0], hp, **win)
    e1 = rel_err(got, np_nlm_layers.nlm_layers(frames[0], layers[0], hp, **win))
    gt = ctx.nlm_layers_temporal(frames, layers, 1, hparam=hp, **win)
    want = chk.nlm_layers_temporal(frames, layers, 1, hp, **win)
    e2 = max(rel_err(a, b) for a, b in zip(gt, want))
    print(f"{cfg} h = {hp}: HDR one frame {e1:.2e}, two frames {e2:.2e}")
    assert e1 < TOL and e2 < TOL, (cfg, hp, e1, e2)
    # the same frames as RGBA16F: the bits of the float32 frames they widen to
    half = [f.astype(np.float16) for f in frames]
    assert all(np.array_equal(a.astype(np.float32), b) for a, b in zip(half, frames))
    assert np.array_equal(bits(ctx.nlm_layers(half[0], layers[0], hp, **win)), bits(got))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ctx.nlm_layers_temporal(half, layers, 1, hparam=hp, **win), gt))


@pytest.mark.parametrize("cfg", STRIP + ("generic",))
def test_rgba8_input_against_the_checker(ctx, cfg):
    rng = np.random.default_rng(32)
    h, w = 70, 150
    win = NLM_CFGS[cfg]
    _, layers = sequence(rng, h, w, 2, 2)
    u8 = [np.clip(noisy(rng, h, w, translucent=True) * 255, 0, 255).astype(np.uint8) for _ in range(2)]
    e1 = rel_err(ctx.nlm_layers(u8[0], layers[0], H, **win), np_nlm_layers.nlm_layers(u8[0], layers[0], H, **win))
    e2 = max(rel_err(a, b) for a, b in zip(ctx.nlm_layers_temporal(u8, layers, 1, hparam=H, **win),
                                           chk.nlm_layers_temporal(u8, layers, 1, H, **win)))
    print(f"{cfg}: RGBA8 one frame {e1:.2e}, two frames {e2:.2e}")
    assert e1 < TOL and e2 < TOL


# ---- d. non-finite texels --------------------------------------------------------------------------------------------------------
def same_masks_and_values(got, want, what):
    """The NaN, +Inf and -Inf masks of the checker, every other value within TOL; returns the worst of those."""
    got = np.asarray(got, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN mask")
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), (what, "+Inf mask")
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), (what, "-Inf mask")
    fin = np.isfinite(want)
    e = rel_err(got[fin], want[fin])
    assert e < TOL, (what, e)
    return e


@pytest.mark.parametrize("cfg", STRIP + ("generic",))
@pytest.mark.parametrize("dtype", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("guide", ["step", "flat"])
def test_nan_and_inf_texels_propagate_like_the_checker(ctx, cfg, dtype, guide):
    # Guides of 0 and 255 only, h = 0.05: one mismatching texel gives exp(-1200), 0 in fp32 and in float64, so every weight is exactly
    # 0 or 1 in both and no flushed tiny weight separates Inf * 0 = NaN from Inf * tiny = Inf.  (With the flat guide the weights are 0
    # where a patch reaches beyond the frame, whose texels are 0.)
    rng = np.random.default_rng(41)
    h, w, xe, hp = 70, 150, 75, 0.05
    win = NLM_CFGS[cfg]
    g = np.full((h, w, 4), 255, np.uint8)
    if guide == "step":
        g[:, :xe, :3] = 0
    clean = noisy(rng, h, w).astype(dtype)
    bad = noisy(rng, h, w).astype(dtype)
    bad[1, 2, :3] = np.inf          # near a frame corner (alpha stays 1)
    bad[30, xe - 1] = -np.inf       # beside the guide's step, all four channels
    bad[66, 100, 1] = np.nan        # in the second tile row and column of both strip kernels
    with np.errstate(all="ignore"):
        want = np_nlm_layers.nlm_layers(bad, [g, g], hp, **win)
        want_t = chk.nlm_layers_temporal([clean, bad], [[g], [g]], 1, hp, **win)
    assert np.isnan(want).any() and np.isposinf(want).any() and np.isneginf(want).any() and np.isfinite(want).any()
    got = ctx.nlm_layers(bad, [g, g], hp, **win)
    e1 = same_masks_and_values(got, want, (cfg, guide, "one frame"))
    W = np.zeros((h, w, 8), np.float32)
    for _ in range(2):
        W = ctx.nlm_layers_accum(bad, g, W, hp, **win)
    assert np.array_equal(bits(got), bits(ctx.normalize(W))), (cfg, guide, "fused == accumulate chain")
    # over frames: the non-finite texels in the neighbour only, so output 0 owes them to frame 1
    got_t = ctx.nlm_layers_temporal([clean, bad], [[g], [g]], 1, hparam=hp, **win)
    assert not np.isfinite(want_t[0]).all()
    e2 = max(same_masks_and_values(got_t[t], want_t[t], (cfg, guide, "output", t)) for t in range(2))
    for t in range(2):
        assert np.array_equal(bits(got_t[t]), bits(chain(ctx, [clean, bad], [[g], [g]], 1, t, win, hp))), (cfg, guide, t)
    print(f"{cfg} {guide} {np.dtype(dtype).name}: finite values {e1:.2e} / {e2:.2e}; "
          f"{int(np.isnan(want).sum())} NaN, {int(np.isinf(want).sum())} Inf, {int(np.isfinite(want).sum())} finite")


# ---- e. the guide's alpha is not read --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["ref", "generic"])
def test_the_guides_alpha_byte_is_not_read(ctx, cfg):
    rng = np.random.default_rng(51)
    h, w = 70, 150
    win = NLM_CFGS[cfg]
    frames, layers = sequence(rng, h, w, 2, 2, translucent=True)
    other = [[g.copy() for g in ls] for ls in layers]
    for ls in other:
        for g in ls:
            g[..., 3] = rng.integers(0, 256, (h, w))
    assert all((a[..., 3] != b[..., 3]).any() and np.array_equal(a[..., :3], b[..., :3]) for x, y in zip(layers, other) for a, b in zip(x, y))
    assert np.array_equal(bits(ctx.nlm_layers(frames[0], layers[0], H, **win)), bits(ctx.nlm_layers(frames[0], other[0], H, **win)))
    W = (rng.random((h, w, 8)) + 0.5).astype(np.float32)
    assert np.array_equal(bits(ctx.nlm_layers_accum(frames[0], layers[0][0], W, H, **win)),
                          bits(ctx.nlm_layers_accum(frames[0], other[0][0], W, H, **win)))
    # the pair form: the target's alpha, the neighbour's alpha, both
    want = bits(ctx.nlm_layers_pair_accum(layers[0][0], layers[1][0], frames[1], W, H, **win))
    for gt, gn in ((other[0][0], layers[1][0]), (layers[0][0], other[1][0]), (other[0][0], other[1][0])):
        assert np.array_equal(bits(ctx.nlm_layers_pair_accum(gt, gn, frames[1], W, H, **win)), want)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ctx.nlm_layers_temporal(frames, layers, 1, hparam=H, **win),
                                                                  ctx.nlm_layers_temporal(frames, other, 1, hparam=H, **win)))
