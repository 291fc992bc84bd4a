"""GPU suite: NLM search windows up to the ABI's limit of 64, on both sides of every boundary between the kernels that serve them
(tests/np_nlm_match.py WIDE_CASES: 4-wave tile, 8-wave tile, 4-wave tile of more than 80 KB, 4-row strips, the per-pixel kernel),
and the layer-guided filters at their window limits.

The NLM cases run on 0/1-weight frames (tests/np_nlm_match.py): every weight is exactly 0 or 1, so the sums have exact known answers
at any window size -- the alpha sum names the offsets that were visited and matched, and tests/test_nlm_match_reference.py shows on
the same frames that a kernel off by one search row or column, or one patch row or column, would change it at many pixels.  (An
fp32 tolerance that grows with the number of offsets cannot tell one missing offset of 4096 from rounding.)"""
import numpy as np
import pytest

import f64_checker
import np_nlm_layers
import np_nlm_match as npm
from conftest import rel_err, synth_hdr

pytestmark = pytest.mark.gpu

H = npm.EXACT_H
NLM_TOL = 2e-5
TEMPORAL = [c for c in npm.WIDE_CASES if c[3]]


def _w0(rng, h, w):
    """A nonzero W to accumulate into: integer colour sums (exact sums stay exact), a fractional normWeight, random pad words."""
    W0 = np.empty((h, w, 8), np.float32)
    W0[..., :4] = rng.integers(0, 16, (h, w, 4))
    W0[..., 4] = rng.random((h, w), dtype=np.float32) * 4
    W0[..., 5:] = rng.standard_normal((h, w, 3))
    return W0


def _ulps(got, want):
    want = np.asarray(want, np.float32)
    return np.abs(np.asarray(got, np.float64) - want) / np.spacing(np.abs(want)).astype(np.float64)


def _check_accum(Wg, W0, num, count, label, rgb_bound=None):
    want = W0[..., :4].astype(np.float64) + num
    assert np.array_equal(Wg[..., 3].astype(np.float64), want[..., 3]), f"{label}: alpha = W0 + the sum over the matching offsets"
    if rgb_bound is None:
        assert np.array_equal(Wg[..., :3].astype(np.float64), want[..., :3]), f"{label}: rgb = W0 + the matching offsets' colours"
    else:
        assert np.all(np.abs(Wg[..., :3] - want[..., :3]) <= rgb_bound), label
    nw = (W0[..., 4] + npm.fp32_norm(count[None])).astype(np.float32)
    assert _ulps(Wg[..., 4], nw).max() <= 2, f"{label}: normWeight = W0 + 0.001 + count"
    assert np.array_equal(Wg[..., 5:].view(np.uint32), W0[..., 5:].view(np.uint32)), f"{label}: the pad words are never written"


@pytest.mark.parametrize("case", npm.WIDE_CASES, ids=npm.case_id)
def test_accumulate_exact_sums(ctx, case):
    search, patch = case[:2]
    h, w = npm.CASE_SHAPE
    rng = np.random.default_rng(5)
    W0 = _w0(rng, h, w)
    t, nb = npm.case_pair(case)
    num, count = npm.match_sums(t, nb, search, patch)
    for dt in (np.float32, np.float16):                   # palette colours and alpha codes are exact in both
        Wg = ctx.nlm_accum(t.astype(dt), nb.astype(dt), W0, H, search, patch)
        _check_accum(Wg, W0, num, count, np.dtype(dt).name)
    # RGBA8: alpha is 0 or 1.0 (exact sums); rgb sums count copies of one fp32 value c/255: within count x 2^-24 of the exact sum,
    # which stays below one matching offset's contribution (>= 64/255) as long as count^2 < 2^24 * 64/192
    t8, nb8 = npm.case_pair(case, u8=True)
    num8, count8 = npm.match_sums(t8, nb8, search, patch)
    want = W0[..., :3].astype(np.float64) + num8[..., :3]
    bound = (count8[..., None] + 1) * 2.0 ** -24 * num8[..., :3] + np.spacing(want.astype(np.float32))
    assert bound.max() < 64 / 255
    _check_accum(ctx.nlm_accum(t8, nb8, W0, H, search, patch), W0, num8, count8, "rgba8", rgb_bound=bound)


@pytest.mark.parametrize("case", TEMPORAL, ids=npm.case_id)
def test_temporal_exact_and_equal_to_the_accumulate_chain(ctx, case):
    """k = 0 and k = 1 over five frames (neighbours clipped at the ends): each output is fp32(num) / fp32(norm) of the exact sums,
    bit for bit the chain of accumulate dispatches + normalize, and a sub-range sees the same neighbour frames."""
    search, patch = case[:2]
    h, w = npm.CASE_SHAPE
    frames = npm.case_frames(case)
    n, cache = len(frames), {}
    for k in (0, 1):
        fused = ctx.nlm_temporal(frames, k=k, hparam=H, search=search, patch=patch)
        for t in range(n):
            num, counts = npm.temporal_sums(frames, t, k, search, patch, cache)
            assert _ulps(fused[t], npm.normalized_fp32(num, counts)).max() <= 2, (k, t)
            W = np.zeros((h, w, 8), np.float32)
            for f in range(max(0, t - k), min(n - 1, t + k) + 1):
                W = ctx.nlm_accum(frames[t], frames[f], W, H, search, patch)
            assert np.array_equal(fused[t], ctx.normalize(W)), (k, t)
        part = ctx.nlm_temporal(frames, k=k, first=1, count=3, hparam=H, search=search, patch=patch)
        assert all(np.array_equal(part[i], fused[1 + i]) for i in range(3)), k


@pytest.mark.parametrize("search,patch", [(npm.sym(52), npm.P7), (npm.sym(64), npm.P7)], ids=["4w>80K", "generic"])
def test_translation_moves_the_output(ctx, search, patch):
    """A pixel's bits depend neither on its wave, tile and lane nor on the kernel's launch form: the frame shifted by 8 rows and
    5 columns gives the shifted output, and fused == accumulate + normalize (smooth HDR content, h = 0.5)."""
    rng = np.random.default_rng(search[1])
    h, w = 150, 160
    t = (synth_hdr(rng, h, w) * 0.25).astype(np.float32)
    fused = ctx.nlm_temporal([t], k=0, search=search, patch=patch)[0]
    assert np.array_equal(fused, ctx.normalize(ctx.nlm_accum(t, t, np.zeros((h, w, 8), np.float32), 0.5, search, patch)))
    halo = -search[0] + max(-patch[0], patch[1])
    shifted = ctx.nlm_temporal([np.ascontiguousarray(t[8:, 5:])], k=0, search=search, patch=patch)[0]
    assert np.array_equal(shifted[halo:-halo, halo:-halo], fused[8 + halo:-halo, 5 + halo:-halo])


def test_sequence_nlm_at_the_widest_window_is_the_temporal_call(ctx):
    case = next(c for c in npm.WIDE_CASES if c[0] == npm.sym(64) and c[1] == npm.P7)
    frames = npm.case_frames(case)
    want = ctx.nlm_temporal(frames, k=1, hparam=H, search=case[0], patch=case[1])
    got, _ = ctx.sequence_nlm(frames, k=1, hparam=H, search=case[0], patch=case[1])
    assert len(got) == len(want)
    for i, (g, w_) in enumerate(zip(got, want)):
        assert np.array_equal(g, w_), i


def test_smooth_hdr_frame_at_the_widest_window_against_float64(ctx):
    """Real content is no worse than the 0/1 frames: 64x64 offsets, weights of every size, held against the float64 checker with
    the tolerance scaled by the number of offsets (test_gpu_parity.test_nlm_unusual_windows)."""
    rng = np.random.default_rng(64)
    h, w = 60, 90
    t = (synth_hdr(rng, h, w) * 0.25).astype(np.float32)
    nb = (t * rng.gamma(16.0, 1 / 16.0, (h, w, 1))).astype(np.float32)
    search, patch = npm.sym(64), npm.P7
    got = ctx.nlm_accum(t, nb, np.zeros((h, w, 8), np.float32), 0.5, search, patch)
    num, den = f64_checker.nlm_sums(t, [nb], 0.5, search, patch)
    ref = np.concatenate([num.cpu().numpy(), den.cpu().numpy()[..., None]], -1)
    assert rel_err(got[..., :5], ref) < NLM_TOL * 4096 / 441


# ---- layer-guided NLM: every window but the two tuned ones runs nlm_layers_generic_kernel ----------------------------------------
PALETTE_G = np.array([(r, g, b) for r in (128, 255) for g in (128, 255) for b in (128, 255)], np.uint8)
LAYER_H = 0.04


def _coord_image(h, w):
    """Input colours that are small integer codes of the texel's coordinates: their sums over any set of offsets are exact."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([xx + 1, yy + 1, (xx * 7 + yy * 3) % 32 + 1, np.ones_like(xx)], -1).astype(np.float32)


@pytest.mark.parametrize("patch", [npm.P7, npm.P16], ids=["7x7", "16x16"])
def test_layers_widest_window_exact(ctx, patch):
    """0/1-weight guides (bytes {128, 255}: one differing texel puts the exponent below -150 at h = 0.04), input colours that are
    coordinate codes: the accumulate sums are exact, the fused output is within two ulp of fp32(num) / fp32(norm) and of float64."""
    search = npm.sym(64)
    kd = np.float32(npm.LOG2E / (float(np.float32(LAYER_H)) ** 2 * 255.0 ** 2))
    assert 127 ** 2 * float(kd) > 150
    rng = np.random.default_rng(patch[1])
    h, w = npm.CASE_SHAPE
    base = npm.pattern_frame(rng, h, w, search, PALETTE_G)
    gl = [npm.with_defects(rng, base, h * w // 400, PALETTE_G) for _ in range(2)]
    img = _coord_image(h, w)
    sums = [npm.match_sums(g, g, search, patch, colour=img) for g in gl]
    W0 = _w0(rng, h, w)
    _check_accum(ctx.nlm_layers_accum(img, gl[0], W0, LAYER_H, search, patch), W0, sums[0][0], sums[0][1], "layer 0")
    out = ctx.nlm_layers(img, gl, LAYER_H, search, patch)
    num, counts = sums[0][0] + sums[1][0], np.stack([s[1] for s in sums])
    assert _ulps(out, npm.normalized_fp32(num, counts)).max() <= 2
    assert _ulps(out, num / (counts.sum(0) + 0.002)[..., None]).max() <= 2


def test_layers_large_h_16x16_patch_against_float64(ctx):
    """Patch distances past 2^24 (a 16x16 patch of bytes sums to up to 3 * 256 * 255^2), where fp32 no longer holds them exactly,
    with h large enough that those offsets still weigh: the fused output against the float64 checker."""
    rng = np.random.default_rng(1616)
    h, w, hp = 40, 70, 16.0
    search, patch = npm.sym(64), npm.P16
    yy, xx = np.mgrid[0:h, 0:w]
    gl = []
    for i in range(2):
        g = np.repeat((255 * ((xx + yy + i) % 2))[..., None], 4, -1) + rng.integers(-6, 7, (h, w, 4))
        gl.append(np.clip(g, 0, 255).astype(np.uint8))
    g0 = gl[0][..., :3].astype(np.int64)
    assert ((g0[10:26, 10:26] - g0[10:26, 11:27]) ** 2).sum() > 2 ** 24
    img = (synth_hdr(rng, h, w) * 0.25).astype(np.float32)
    got = ctx.nlm_layers(img, gl, hp, search, patch)
    want = np_nlm_layers.nlm_layers(img, gl, hp, search, patch)
    assert rel_err(got, want) < NLM_TOL * 4096 / 441
