"""GPU suite, maximum sizes: mid_firefly_clamp (section a4l) on ONE frame whose output passes 4 GiB.

16400 x 16400: a u8 frame tiled from a 37 x 41 pattern on the device, clamped at radius 2 into a 4.3 GB RGBA32F plane that holds
NaN before the call; 257 x 1025 tiles, dealt to the launch's capped grid.  Crops at the four corners and across the 4 GiB byte
offset of the output (pixel 2^28: row 16368, column 256) against tests/np_firefly.py on the crop grown by the radius and cut at the
frame's edge, bit for bit.  Memory is handled exactly as tests/test_gpu_huge_frame.py handles it: the buffers are allocated, and
released at the end.
"""
import ctypes

import numpy as np
import pytest
import torch

import image_denoising_filter_amd as mid
import np_firefly as chk
from test_gpu_atrous_bounds import bits

pytestmark = pytest.mark.gpu
H, W = 16400, 16400
PH, PW = 37, 41
RADIUS, RANK, SIZE = 2, 2, 24


def test_one_frame_beyond_4_gib(ctx):
    assert H * W * 16 > 2 ** 32 and H * W < 2 ** 30
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)                       # (one explicit stream for torch's fills and the kernel: a NULL stream is the context's own)
    pat = np.random.default_rng(80).integers(0, 256, (PH, PW, 4), dtype=np.uint8)
    with torch.cuda.stream(ts):
        fr = torch.from_numpy(pat).to(dev).repeat(-(-H // PH), -(-W // PW), 1)[:H, :W].contiguous()
        out = torch.full((H, W, 4), float("nan"), device=dev, dtype=torch.float32)
    s = ts.cuda_stream
    assert s != 0
    p = mid.FireflyParams(W, H, RADIUS, RANK, 1.0, 0.0, mid.FMT_RGBA8)
    assert mid.lib.mid_firefly_clamp(ctx.handle, ctypes.byref(p), fr.data_ptr(), out.data_ptr(), s) == 0, mid.lib.mid_last_error()
    torch.cuda.synchronize()
    row, col = 2 ** 28 // W, 2 ** 28 % W
    assert (row, col) == (16368, 256)
    changed = 0
    for y0, x0 in ((0, 0), (0, W - SIZE), (H - SIZE, 0), (H - SIZE, W - SIZE), (row - 2, col - 12), (row, 0), (row - 1, W - SIZE)):
        ya, xa = max(0, y0 - RADIUS), max(0, x0 - RADIUS)                        # the crop grown by the radius, cut at the frame's edge
        yb, xb = min(H, y0 + SIZE + RADIUS), min(W, x0 + SIZE + RADIUS)
        crop = pat[np.ix_(np.arange(ya, yb) % PH, np.arange(xa, xb) % PW)]
        assert np.array_equal(fr[ya:yb, xa:xb].cpu().numpy(), crop)
        c = {}
        want = chk.firefly_clamp(crop, RADIUS, RANK, 1.0, 0.0, counts=c)[y0 - ya:y0 - ya + SIZE, x0 - xa:x0 - xa + SIZE]
        changed += c["clamped"]
        got = out[y0:y0 + SIZE, x0:x0 + SIZE].cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (y0, x0)
    assert changed > 0
    assert not bool(torch.isnan(out[-1]).any()) and not bool(torch.isnan(out[::997]).any())     # every sampled row was written
    del fr, out
    torch.cuda.empty_cache()
