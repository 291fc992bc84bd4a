"""GPU suite, maximum sizes: mid_guided_filter (section a4o) on ONE frame whose output passes 4 GiB.

16400 x 16400: a u8 frame and a u8 guide tiled from two 37 x 41 patterns on the device, radius 2, into a 4.3 GB RGBA32F plane that holds
NaN before the call, through a 14 GB workspace; 66 x 513 tiles, dealt to the launch's capped grid.  Crops at the four corners and across
the 4 GiB byte offset of the output (pixel 2^28: row 16368, column 256) against tests/np_guided.py on the crop grown by twice the
radius -- a pixel reads the models of its window, a model the texels of its own -- and cut at the frame's edge, to the header's
bound.  Memory is handled exactly as tests/test_gpu_huge_frame.py handles it: the buffers are allocated, and released at the end.
"""
import ctypes

import numpy as np
import pytest
import torch

import image_denoising_filter_amd as mid
import np_guided

pytestmark = pytest.mark.gpu
H, W = 16400, 16400
PH, PW = 37, 41
RADIUS, EPS, SIZE = 2, 1e-3, 24       # u8 texels: D <= 1, n_min = 9, so D^2 / eps = 1000 <= 2^10 * 9


def test_one_frame_beyond_4_gib(ctx):
    assert H * W * 16 > 2 ** 32 and H * W < 2 ** 30
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)                       # (one explicit stream for torch's fills and the kernels: a NULL stream is the context's own)
    rng = np.random.default_rng(83)
    pat, gpat = rng.integers(0, 256, (PH, PW, 4), dtype=np.uint8), rng.integers(0, 256, (PH, PW, 4), dtype=np.uint8)
    p = mid.GuidedParams(W, H, RADIUS, EPS, mid.api.fmt_with_guide(mid.FMT_RGBA8, mid.FMT_RGBA8))
    n = ctypes.c_size_t()
    assert mid.lib.mid_guided_workspace(ctypes.byref(p), ctypes.byref(n)) == 0 and n.value == 52 * H * W
    with torch.cuda.stream(ts):
        fr = torch.from_numpy(pat).to(dev).repeat(-(-H // PH), -(-W // PW), 1)[:H, :W].contiguous()
        gd = torch.from_numpy(gpat).to(dev).repeat(-(-H // PH), -(-W // PW), 1)[:H, :W].contiguous()
        out = torch.full((H, W, 4), float("nan"), device=dev, dtype=torch.float32)
        work = torch.empty((n.value,), device=dev, dtype=torch.uint8)
    s = ts.cuda_stream
    assert s != 0
    rc = mid.lib.mid_guided_filter(ctx.handle, ctypes.byref(p), fr.data_ptr(), gd.data_ptr(), work.data_ptr(), out.data_ptr(), mid.FMT_RGBA32F, s)
    assert rc == 0, mid.lib.mid_last_error()
    torch.cuda.synchronize()
    row, col = 2 ** 28 // W, 2 ** 28 % W
    assert (row, col) == (16368, 256)
    worst, reach = 0.0, 2 * RADIUS
    for y0, x0 in ((0, 0), (0, W - SIZE), (H - SIZE, 0), (H - SIZE, W - SIZE), (row - 2, col - 12), (row, 0), (row - 1, W - SIZE)):
        ya, xa = max(0, y0 - reach), max(0, x0 - reach)
        yb, xb = min(H, y0 + SIZE + reach), min(W, x0 + SIZE + reach)
        ix = np.ix_(np.arange(ya, yb) % PH, np.arange(xa, xb) % PW)
        assert np.array_equal(fr[ya:yb, xa:xb].cpu().numpy(), pat[ix]) and np.array_equal(gd[ya:yb, xa:xb].cpu().numpy(), gpat[ix])
        ref = np_guided.guided(pat[ix], gpat[ix], RADIUS, EPS)
        cut = (slice(y0 - ya, y0 - ya + SIZE), slice(x0 - xa, x0 - xa + SIZE))
        got = out[y0:y0 + SIZE, x0:x0 + SIZE].cpu().numpy()
        assert ref["filtered"][cut].all()
        err = np.abs(got[..., :3].astype(np.float64) - ref["out"][cut][..., :3]) / np_guided.tolerance(ref)[cut]
        assert np.array_equal(got[..., 3].astype(np.float64), ref["out"][cut][..., 3]), (y0, x0, "alpha")
        worst = max(worst, float(err.max()))
    print(f"16400 x 16400: worst error {worst:.3f} of the tolerance")
    assert worst <= 1.0
    assert not bool(torch.isnan(out).any())                                      # no NaN is left: every pixel was written
    del fr, gd, out, work
    torch.cuda.empty_cache()
