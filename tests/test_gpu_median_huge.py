"""GPU suite, maximum sizes: mid_median_filter (section a4p) on ONE frame whose output passes 4 GiB -- the smallest frame at which
32-bit index arithmetic can go wrong.

16400 x 16400: a u8 frame and a u8 guide tiled from two 37 x 41 patterns on the device, radius 1, one layer, into a 4.3 GB RGBA32F
plane that holds NaN before the call; 257 x 1025 tiles, dealt to the launch's capped grid.  Bands of rows at the top, at the bottom and
across the 4 GiB byte offset of the output (pixel 2^28: row 16368, column 256) against tests/np_median.py on the band grown by the
radius and cut at the frame's edge, by the acceptance rule of the header.  Then the same call with four all-zero layers more, which
runs the global class (one pixel per lane, its own tap addresses, a 257 x 4100 grid) over the whole frame: every pixel equal.  Memory is handled exactly as
tests/test_gpu_huge_frame.py handles it: the buffers are allocated, and released at the end.
"""
import ctypes

import numpy as np
import pytest
import torch

import image_denoising_filter_amd as mid
import median_inputs as mi
import np_median

pytestmark = pytest.mark.gpu
H, W = 16400, 16400
PH, PW = mi.HUGE_PATTERN
RADIUS, SIGMA, ROWS = 1, mi.HUGE_SIGMA, 3


def test_one_frame_beyond_4_gib(ctx):
    assert H * W * 16 > 2 ** 32 and H * W < 2 ** 30
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)                       # (one explicit stream for torch's fills and the kernel: a NULL stream is the context's own)
    pat, gpat = mi.huge_patterns()
    p = mid.MedianParams(W, H, RADIUS, mid.FMT_RGBA8)
    with torch.cuda.stream(ts):
        fr = torch.from_numpy(pat).to(dev).repeat(-(-H // PH), -(-W // PW), 1)[:H, :W].contiguous()
        gd = torch.from_numpy(gpat).to(dev).repeat(-(-H // PH), -(-W // PW), 1)[:H, :W].contiguous()
        out = torch.full((H, W, 4), float("nan"), device=dev, dtype=torch.float32)
    s = ts.cuda_stream
    assert s != 0
    rc = mid.lib.mid_median_filter(ctx.handle, ctypes.byref(p), (ctypes.c_float * 1)(SIGMA), fr.data_ptr(), (ctypes.c_void_p * 1)(gd.data_ptr()), 1,
                                   out.data_ptr(), mid.FMT_RGBA32F, s)
    assert rc == 0, mid.lib.mid_last_error()
    torch.cuda.synchronize()
    row, col = 2 ** 28 // W, 2 ** 28 % W
    assert (row, col) == (16368, 256)
    near = 0.0
    for y0 in (0, row - 1, H - ROWS):                        # whole rows: both frame edges, every tile column
        ya, yb = max(0, y0 - RADIUS), min(H, y0 + ROWS + RADIUS)
        ix = np.ix_(np.arange(ya, yb) % PH, np.arange(W) % PW)
        frame, guide = pat[ix], gpat[ix]
        assert np.array_equal(fr[ya:yb].cpu().numpy(), frame) and np.array_equal(gd[ya:yb].cpu().numpy(), guide)
        cut = slice(y0 - ya, y0 - ya + ROWS)
        grown = np.zeros((yb - ya, W, 4), np.float32)
        grown[cut] = out[y0:y0 + ROWS].cpu().numpy()
        res = np_median.accept(grown, frame, [guide], [SIGMA], RADIUS)
        assert not res["bad"][cut].any(), y0
        assert np.array_equal(grown[cut][..., 3], frame[cut][..., 3].astype(np.float32) / np.float32(255)), (y0, "alpha")
        near = max(near, res["near"])
    print(f"16400 x 16400: at most {near:.4f} of a band's pixel-channels held to the inequalities")
    assert not bool(torch.isnan(out).any())                                      # no NaN is left: every pixel was written
    # the global class (its own tap addresses, a 257 x 4100 grid) across the same offset: four all-zero layers more send the call there,
    # and leave the values of every pixel
    with torch.cuda.stream(ts):
        zero = torch.zeros((H, W, 4), device=dev, dtype=torch.uint8)
        out5 = torch.full((H, W, 4), float("nan"), device=dev, dtype=torch.float32)
    rc = mid.lib.mid_median_filter(ctx.handle, ctypes.byref(p), (ctypes.c_float * 5)(SIGMA, 1.0, 1.0, 1.0, 1.0), fr.data_ptr(),
                                   (ctypes.c_void_p * 5)(gd.data_ptr(), *[zero.data_ptr()] * 4), 5, out5.data_ptr(), mid.FMT_RGBA32F, s)
    assert rc == 0, mid.lib.mid_last_error()
    torch.cuda.synchronize()
    assert bool(torch.equal(out5, out))                                          # (no NaN on either side, as shown above)
    del fr, gd, out, zero, out5
    torch.cuda.empty_cache()
