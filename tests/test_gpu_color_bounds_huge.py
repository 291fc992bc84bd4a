"""GPU suite, maximum sizes: mid_color_bounds (section a4m) on ONE frame whose outputs pass 4 GiB.

16400 x 16400: a u8 frame tiled from a 37 x 41 pattern on the device, its box at radius 2 into two 4.3 GB RGBA32F planes that hold NaN
before the call; 257 x 1025 tiles, dealt to the launch's capped grid.  Crops at the four corners and across the 4 GiB byte offset
of the outputs (pixel 2^28: row 16368, column 256) against tests/np_color_bounds.py on the crop grown by the radius and cut at the
frame's edge, with test_gpu_color_bounds.py's tolerance; the counts exact.  Memory is handled exactly as tests/test_gpu_huge_frame.py
handles it: the buffers are allocated, and released at the end.
"""
import ctypes

import numpy as np
import pytest
import torch

import image_denoising_filter_amd as mid
from np_color_bounds import color_bounds as check

pytestmark = pytest.mark.gpu
H, W = 16400, 16400
PH, PW = 37, 41
RADIUS, GAMMA, SIZE = 2, 1.0, 24


def test_one_frame_beyond_4_gib(ctx):
    assert H * W * 16 > 2 ** 32 and H * W < 2 ** 30
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)                       # (one explicit stream for torch's fills and the kernel: a NULL stream is the context's own)
    pat = np.random.default_rng(81).integers(0, 256, (PH, PW, 4), dtype=np.uint8)
    with torch.cuda.stream(ts):
        fr = torch.from_numpy(pat).to(dev).repeat(-(-H // PH), -(-W // PW), 1)[:H, :W].contiguous()
        lo = torch.full((H, W, 4), float("nan"), device=dev, dtype=torch.float32)
        hi = torch.full((H, W, 4), float("nan"), device=dev, dtype=torch.float32)
    s = ts.cuda_stream
    assert s != 0
    p = mid.ColorBoundsParams(W, H, RADIUS, GAMMA, mid.FMT_RGBA8)
    assert mid.lib.mid_color_bounds(ctx.handle, ctypes.byref(p), fr.data_ptr(), lo.data_ptr(), hi.data_ptr(), s) == 0, mid.lib.mid_last_error()
    torch.cuda.synchronize()
    row, col = 2 ** 28 // W, 2 ** 28 % W
    assert (row, col) == (16368, 256)
    worst = 0.0
    for y0, x0 in ((0, 0), (0, W - SIZE), (H - SIZE, 0), (H - SIZE, W - SIZE), (row - 2, col - 12), (row, 0), (row - 1, W - SIZE)):
        ya, xa = max(0, y0 - RADIUS), max(0, x0 - RADIUS)                        # the crop grown by the radius, cut at the frame's edge
        yb, xb = min(H, y0 + SIZE + RADIUS), min(W, x0 + SIZE + RADIUS)
        crop = pat[np.ix_(np.arange(ya, yb) % PH, np.arange(xa, xb) % PW)]
        assert np.array_equal(fr[ya:yb, xa:xb].cpu().numpy(), crop)
        sc = {}
        want = check(crop, RADIUS, GAMMA, scale=sc)
        cut = (slice(y0 - ya, y0 - ya + SIZE), slice(x0 - xa, x0 - xa + SIZE))
        for plane, ref in zip((lo, hi), want):
            got = plane[y0:y0 + SIZE, x0:x0 + SIZE].cpu().numpy()
            assert np.array_equal(got[..., 3], ref[cut][..., 3].astype(np.float32)), (y0, x0, "the counts")
            e = np.abs(got[..., :3].astype(np.float64) - ref[cut][..., :3]) / np.maximum(1.0, sc["scale"][cut])
            worst = max(worst, float(e.max()))
    print(f"16400 x 16400: worst error {worst:.2e} of the tolerance's scale")
    assert worst <= 1e-5
    assert float(lo[0, 0, 3]) == 9 and float(hi[H - 1, W - 1, 3]) == 9 and float(lo[row, col, 3]) == 25
    for plane in (lo, hi):
        assert not bool(torch.isnan(plane).any())                                # no NaN is left: every pixel was written
    del fr, lo, hi
    torch.cuda.empty_cache()
