"""GPU suite, maximum sizes: mid_image_metrics (section a4n) on ONE pair of frames whose second halves lie beyond the 4 GiB offset.

16400 x 16400 RGBA32F: b is a 37 x 41 pattern of integer levels tiled on the device, a is b with differences planted at known pixels --
(0, 0), the pixels on either side of the 4 GiB byte offset (pixel 2^28: row 16368, column 256), the last pixel -- and one NaN texel.
The pointwise sums and the counts are integers, exact in any order, and are compared bit for bit; 257 x 1025 tiles go to 4096
workgroups.  The map on six crops cut at the frame's edges and across the offset against tests/np_image_metrics.py on the crop
grown by the window's radius.  Memory is handled exactly as tests/test_gpu_huge_frame.py handles it."""
import ctypes

import numpy as np
import pytest
import torch

import image_denoising_filter_amd as mid
import np_image_metrics as M

pytestmark = pytest.mark.gpu
H, W = 16400, 16400
PH, PW = 37, 41
SIZE, R = 24, 5


def test_one_pair_beyond_4_gib(ctx):
    assert H * W * 16 > 2 ** 32 and H * W < 2 ** 30
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    pat = np.random.default_rng(83).integers(0, 256, (PH, PW, 4)).astype(np.float32)
    row, col = 2 ** 28 // W, 2 ** 28 % W
    assert (row, col) == (16368, 256)
    planted = {(0, 0): (3.0, 0), (row, col - 1): (-7.0, 1), (row, col): (11.0, 2), (H - 1, W - 1): (-300.0, 0), (row + 1, 70): (0.5, 1)}
    nan_at = (row - 1, W - 3)
    nw = mid.lib.mid_image_metrics_workspace(W, H)
    assert nw == 4097 * 128
    with torch.cuda.stream(ts):
        b = torch.from_numpy(pat).to(dev).repeat(-(-H // PH), -(-W // PW), 1)[:H, :W].contiguous()
        a = b.clone()
        for (y, x), (d, c) in planted.items():
            a[y, x, c] += d
        a[nan_at[0], nan_at[1], 2] = float("nan")
        work = torch.full((nw // 8 + 64,), float("nan"), device=dev, dtype=torch.float64)
        smap = torch.full((H, W), -7.0, device=dev, dtype=torch.float32)
    s = ts.cuda_stream
    assert s != 0
    p = mid.ImageMetricsParams(W, H, mid.FMT_RGBA32F, mid.FMT_RGBA32F, 255.0, 1.0, 1)
    assert mid.lib.mid_image_metrics(ctx.handle, ctypes.byref(p), a.data_ptr(), b.data_ptr(), work.data_ptr(), smap.data_ptr(), s) == 0, mid.lib.mid_last_error()
    torch.cuda.synchronize()
    sums = work[:16].cpu().numpy()
    assert bool(torch.isnan(work[nw // 8:]).all())
    assert sums[M.I_VALID] == H * W - 1 and sums[M.I_INVALID] == 1
    for c in range(3):
        ds = [d for d, cc in planted.values() if cc == c]
        assert sums[M.I_SQ + c] == sum(d * d for d in ds) and sums[M.I_ABS + c] == sum(abs(d) for d in ds), c
    assert sums[M.I_MAX] == 300.0 and not sums[13:].any()
    worst = 0.0
    for y0, x0 in ((0, 0), (0, W - SIZE), (H - SIZE, 0), (H - SIZE, W - SIZE), (row - 2, col - 12), (row - 1, W - SIZE)):
        ya, xa, yb, xb = max(0, y0 - R), max(0, x0 - R), min(H, y0 + SIZE + R), min(W, x0 + SIZE + R)
        ca, cb = a[ya:yb, xa:xb].cpu().numpy(), b[ya:yb, xa:xb].cpu().numpy()
        assert np.array_equal(cb, pat[np.ix_(np.arange(ya, yb) % PH, np.arange(xa, xb) % PW)])
        ref = M.image_metrics(ca, cb, peak=255.0, eps=1.0)
        cut = (slice(y0 - ya, y0 - ya + SIZE), slice(x0 - xa, x0 - xa + SIZE))
        got = smap[y0:y0 + SIZE, x0:x0 + SIZE].cpu().numpy()
        want, v = ref["map"][cut], ref["valid"][cut]
        assert np.array_equal(np.isnan(got), ~v), (y0, x0)
        e = np.abs(got[v].astype(np.float64) - want[v]) / (M.ssim_atol(ref["M"][cut][v], 255.0) + np.abs(want[v]) * 2.0 ** -24)
        worst = max(worst, float(e.max()))
    print(f"16400 x 16400: the map's worst error is {worst:.2e} of its tolerance; sum ssim / n = {sums[M.I_SSIM] / sums[M.I_VALID]!r}")
    assert worst <= 1.0
    assert float(smap[5000, 5000]) == 1.0 and float(smap[H - 1, 0]) == 1.0 and float(smap[0, 0]) < 1.0 and float(smap[H - 1, W - 1]) < 1.0
    assert int(torch.isnan(smap).sum()) == 1 and not bool((smap == -7.0).any())     # every pixel was written
    assert H * W - 1 - 2 * 6 * 121 <= sums[M.I_SSIM] < H * W - 1                     # 1.0 outside the windows of the six planted texels, >= -1 inside
    del a, b, work, smap
    torch.cuda.empty_cache()
