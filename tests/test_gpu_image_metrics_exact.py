"""GPU suite: answers of mid_image_metrics (section a4n) that are known exactly, and its bit identities.

Exact: float frames of integers 0 .. 255 with peak 255 -- sum d^2, sum |d|, max |d| and the counts are integers below 2^53, exact in any
order of addition, and are compared bit for bit against int64 arithmetic.
Identities: metrics(a, a); a and b swapped; a u8 frame and the float frame it widens to; a, b and peak times 2^k with eps times 4^k;
five calls in a row and a call on a second stream; ssim == 0 against ssim == 1."""
import ctypes

import numpy as np
import pytest
import torch

import image_denoising_filter_amd as mid
import np_image_metrics as M
from image_metrics_inputs import pair
from np_albedo import widen

pytestmark = pytest.mark.gpu


def levels(h, w, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 4)).astype(np.float32)
    b = rng.integers(0, 256, (h, w, 4)).astype(np.float32)
    return a, b


@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (16, 64), (17, 65), (37, 131), (70, 300)], ids=lambda s: f"{s[1]}x{s[0]}")
@pytest.mark.parametrize("dt", [np.float32, np.float16], ids=["f32", "f16"])
def test_integer_levels_against_int64(ctx, shape, dt):
    h, w = shape
    a, b = levels(h, w, h * 1000 + w)
    bad = np.zeros((h, w), bool)
    if h * w > 4:
        bad[0, 0] = bad[h - 1, w - 1] = bad[h // 2, w // 3] = True
        a[0, 0, 0], b[h - 1, w - 1, 1], a[h // 2, w // 3, 2] = np.nan, np.inf, -np.inf
    got = ctx.image_metrics(a.astype(dt), b.astype(dt), peak=255.0, ssim=(h % 2 == 1))
    d = np.where(bad[..., None], 0, a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)).astype(np.int64)
    s = got["sums"]
    assert s[M.I_VALID] == (~bad).sum() and s[M.I_INVALID] == bad.sum()
    for c in range(3):
        assert s[M.I_SQ + c] == float((d[..., c] ** 2).sum()), c
        assert s[M.I_ABS + c] == float(np.abs(d[..., c]).sum()), c
    assert s[M.I_MAX] == float(np.abs(d).max())
    n = float((~bad).sum())
    assert got["mse"] == float((d ** 2).sum()) / (3.0 * n) and got["mae"] == float(np.abs(d).sum()) / (3.0 * n)


@pytest.mark.parametrize("shape", [(1, 1), (5, 5), (17, 65), (33, 129)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_an_image_against_itself(ctx, shape):
    h, w = shape
    for scale in (1.0, 700.0, 1e-3):
        a, _ = pair(h, w, scale)
        r = ctx.image_metrics(a, a, peak=scale, eps=1e-2 * scale * scale, want_map=True)
        s = r["sums"]
        assert s[M.I_VALID] == h * w and s[M.I_INVALID] == 0
        assert s[2:12].tobytes() == np.zeros(10).tobytes()                      # every error sum is +0, not -0
        assert s[M.I_SSIM] == h * w                                             # every ssim(p) is exactly 1.0, and so is their sum
        assert np.array_equal(r["map"], np.ones((h, w), np.float32))
        assert r["mse"] == 0 and r["psnr"] == np.inf and r["ssim"] == 1.0 and r["relmse"] == 0 and r["max_abs"] == 0


def test_swapping_the_images(ctx):
    a, b = pair(33, 129)
    a[3, 4, 0] = np.nan
    x, y = ctx.image_metrics(a, b), ctx.image_metrics(b, a)
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 8):
        assert x["sums"][i] == y["sums"][i], i
    assert x["sums"][M.I_REL] != y["sums"][M.I_REL]                             # relMSE is relative to the REFERENCE


def test_a_u8_frame_and_its_widening(ctx):
    a, b = pair(33, 129)
    ua = np.clip(np.rint(a * 255), 0, 255).astype(np.uint8)
    ub = np.clip(np.rint(b * 255), 0, 255).astype(np.uint8)
    fa, fb = widen(ua), widen(ub)
    want = ctx.image_metrics(fa, fb, want_map=True)
    for x, y in ((ua, ub), (ua, fb), (fa, ub)):
        got = ctx.image_metrics(x, y, want_map=True)
        assert got["sums"].tobytes() == want["sums"].tobytes() and got["map"].tobytes() == want["map"].tobytes()
    ha, hb = fa.astype(np.float16), fb.astype(np.float16)                       # and a half frame and ITS widening
    got, want = ctx.image_metrics(ha, hb, want_map=True), ctx.image_metrics(ha.astype(np.float32), hb.astype(np.float32), want_map=True)
    assert got["sums"].tobytes() == want["sums"].tobytes() and got["map"].tobytes() == want["map"].tobytes()


def test_scaling_by_powers_of_two(ctx):
    h, w = 33, 129
    a, b = pair(h, w)
    a[7, 64, 1] = np.inf
    base = ctx.image_metrics(a, b, want_map=True)
    for k in range(-6, 11):
        s = np.float32(2.0 ** k)
        got = ctx.image_metrics(a * s, b * s, peak=float(s), eps=1e-2 * 4.0 ** k, want_map=True)
        assert float(np.float32(1e-2 * 4.0 ** k)) == float(np.float32(1e-2)) * 4.0 ** k
        assert got["map"].tobytes() == base["map"].tobytes(), k                 # every ssim bit
        assert got["sums"][M.I_SSIM] == base["sums"][M.I_SSIM], k
        assert got["sums"][M.I_REL:M.I_REL + 3].tobytes() == base["sums"][M.I_REL:M.I_REL + 3].tobytes(), k
        assert np.array_equal(got["sums"][M.I_SQ:M.I_SQ + 3], base["sums"][M.I_SQ:M.I_SQ + 3] * 4.0 ** k), k
        assert np.array_equal(got["sums"][M.I_ABS:M.I_ABS + 3], base["sums"][M.I_ABS:M.I_ABS + 3] * 2.0 ** k), k
        assert got["sums"][M.I_MAX] == base["sums"][M.I_MAX] * 2.0 ** k and got["relmse"] == base["relmse"] and got["ssim"] == base["ssim"]


def test_repeated_calls_and_a_second_stream(ctx):
    """The bits depend on the inputs and the parameters alone: five calls in a row, and a call on another stream with its own workspace."""
    h, w = 300, 1000                                                            # 19 x 16 tiles: many workgroups in flight
    a, b = pair(h, w)
    first = ctx.image_metrics(a, b, want_map=True)
    for _ in range(4):
        again = ctx.image_metrics(a, b, want_map=True)
        assert again["sums"].tobytes() == first["sums"].tobytes() and again["map"].tobytes() == first["map"].tobytes()
    ts = torch.cuda.Stream(device=torch.device("cuda", 0))
    with torch.cuda.stream(ts):
        da, db = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
        nw = mid.lib.mid_image_metrics_workspace(w, h)
        work = torch.full((nw // 8,), float("nan"), device="cuda:0", dtype=torch.float64)
    ts.synchronize()
    p = mid.ImageMetricsParams(w, h, mid.FMT_RGBA32F, mid.FMT_RGBA32F, 1.0, 1e-2, 1)
    assert ts.cuda_stream != 0
    assert mid.lib.mid_image_metrics(ctx.handle, ctypes.byref(p), da.data_ptr(), db.data_ptr(), work.data_ptr(), None, ts.cuda_stream) == 0, mid.lib.mid_last_error()
    ts.synchronize()
    assert work[:16].cpu().numpy().tobytes() == first["sums"].tobytes()
