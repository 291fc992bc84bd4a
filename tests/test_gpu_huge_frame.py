"""GPU suite, maximum sizes: ONE frame whose buffers pass 4 GiB.

16400 x 16400 RGBA32F = 4,303,360,000 B per colour buffer (> 2^32), its WeightInfo buffer 8.6 GB: every kernel's byte
offsets leave 32 bits (row 16,368 starts beyond 4 GiB, row 8,184 beyond 2 GiB) while pixel indices stay inside `int`.
The frame is built on the device (no 4 GB host array); windows of the results are copied back and compared with the
oracle run on crops around them, as tests/test_gpu_fullsize.py does at 1080p.  Covered: the tuned bilateral tile in
both addressings (the linear one wraps rows, bialteral_linear.comp:58), the fused NLM strip kernel at the benchmark
window, mid_nlm_accum into the 8.6 GB weight buffer + mid_normalize, and pack/unpack over the whole buffer; layer-guided NLM
(mid_nlm_layers fused on the strip and the per-pixel kernel, mid_nlm_layers_accum + mid_normalize, mid_nlm_layers_temporal and its
chain of mid_nlm_layers_pair_accum dispatches) with RGBA8 guides built on the device, against the float64 checkers on crops;
joint layer-guided NLM (mid_nlm_joint) with two guides on its 32-row tiles, into an output that holds NaN before the call.
"""
import ctypes

import numpy as np
import pytest
import torch

import image_denoising_filter_amd as mid
import np_nlm_joint
import np_nlm_layers
import np_nlm_layers_temporal
import oracle
from conftest import rel_err
from test_gpu_nlm_layers import TOL

pytestmark = pytest.mark.gpu
H, W = 16400, 16400
SIZE = 20


def _crop(img_dev, y0, x0, halo):
    """Window + halo as a host array, zero beyond the frame (the texture policy)."""
    ya, yb, xa, xb = y0 - halo, y0 + SIZE + halo, x0 - halo, x0 + SIZE + halo
    out = np.zeros((yb - ya, xb - xa, 4), np.float32)
    sy, sx = slice(max(ya, 0), min(yb, H)), slice(max(xa, 0), min(xb, W))
    out[sy.start - ya:sy.stop - ya, sx.start - xa:sx.stop - xa] = img_dev[sy, sx].cpu().numpy()
    return out


# the far corner, the last rows at the left edge, the rows where byte offsets cross 2 GiB and 4 GiB, the origin
WINDOWS = ((H - SIZE, W - SIZE), (H - SIZE, 0), (8184 - 10, 5000), (16368 - 10, 8000), (16368 - 10, W - SIZE), (0, 0))


@pytest.fixture(scope="module")
def ts():
    """ONE explicit stream for torch's fills and the library's kernels alike.  (A NULL stream argument means the context's own
    compute stream, include/mi_denoise.h:15 -- passing torch's default-stream handle, which IS 0, would let a kernel start
    while the tensor it reads is still being written on torch's stream.)"""
    return torch.cuda.Stream(device=torch.device("cuda", 0))


@pytest.fixture(scope="module")
def huge(ts):
    assert H * W * 16 > 2 ** 32 and H * W < 2 ** 31
    dev = torch.device("cuda", 0)
    with torch.cuda.stream(ts):
        g = torch.Generator(device=dev).manual_seed(90)
        img = torch.rand((H, W, 4), device=dev, generator=g, dtype=torch.float32)
        img[..., :3] *= 0.8
    ts.synchronize()
    yield img
    del img
    torch.cuda.empty_cache()


def test_bilateral_both_addressings_beyond_4_gib(ctx, huge, ts):
    assert ts.cuda_stream != 0
    out = torch.empty_like(huge)
    for layout, orc in ((mid.LAYOUT_TEXTURE, oracle.bilateral_texture), (mid.LAYOUT_LINEAR, oracle.bilateral_linear)):
        ctx.bilateral_dev(huge.data_ptr(), out.data_ptr(), W, H, 8, 2.0, 0.2, layout, mid.FMT_RGBA32F, ts.cuda_stream)
        torch.cuda.synchronize()
        for y0, x0 in WINDOWS:
            if layout == mid.LAYOUT_LINEAR and (x0 < 8 or x0 + SIZE > W - 8):
                continue        # (row ends of the flat addressing see the neighbouring rows: covered at 1080p with whole rows)
            ref = orc(_crop(huge, y0, x0, 8), 8, 2.0, 0.2)[8:8 + SIZE, 8:8 + SIZE]
            assert rel_err(out[y0:y0 + SIZE, x0:x0 + SIZE].cpu().numpy(), ref) < 1e-5, (layout, y0, x0)
    # flat addressing at the very end of the buffer: the last rows, whole width, against the oracle on those rows
    rows = huge[H - 40:].cpu().numpy()
    ref = oracle.bilateral_linear(rows, 8, 2.0, 0.2)
    got = out[H - 40:].cpu().numpy()
    assert rel_err(got[10:, :64], ref[10:, :64]) < 1e-5 and rel_err(got[10:, -64:], ref[10:, -64:]) < 1e-5
    del out


def test_nlm_fused_and_accumulate_normalize_beyond_4_gib(ctx, huge, ts):
    search, patch, halo = (-10, 11), (-3, 4), 14
    s = ts.cuda_stream
    out = torch.empty_like(huge)
    ctx.nlm_temporal_dev([huge.data_ptr()], [out.data_ptr()], W, H, 0.5, search, patch, 0, 0, 1, mid.FMT_RGBA32F, s)
    # the unfused pair the reference dispatches: nonlocal.comp into the 32-byte-stride weight buffer, then normalize.comp
    with torch.cuda.stream(ts):
        Wb = torch.zeros((H, W, 8), device=huge.device, dtype=torch.float32)      # (the fill is ordered before the accumulate: same stream)
    assert Wb.numel() * 4 > 2 ** 33
    out2 = torch.empty_like(huge)
    p = mid.NlmParams(W, H, 0.5, search[0], search[1], patch[0], patch[1], mid.FMT_RGBA32F)
    assert mid.lib.mid_nlm_accum(ctx.handle, ctypes.byref(p), huge.data_ptr(), huge.data_ptr(), Wb.data_ptr(), s) == 0, mid.lib.mid_last_error()
    q = mid.NormalizeParams(W, H)
    assert mid.lib.mid_normalize(ctx.handle, ctypes.byref(q), Wb.data_ptr(), out2.data_ptr(), s) == 0, mid.lib.mid_last_error()
    torch.cuda.synchronize()
    for y0, x0 in WINDOWS:
        c = _crop(huge, y0, x0, halo)
        Wo = oracle.nlm_accum(c, c, np.zeros(c.shape[:2] + (8,), np.float32), 0.5, search=search, patch=patch)
        ref = oracle.normalize(Wo)[halo:halo + SIZE, halo:halo + SIZE]
        a = out[y0:y0 + SIZE, x0:x0 + SIZE].cpu().numpy()
        b = out2[y0:y0 + SIZE, x0:x0 + SIZE].cpu().numpy()
        assert rel_err(a, ref) < 2e-5, (y0, x0)
        assert np.array_equal(a, b), "fused == accumulate + normalize, bit for bit"
        wgot = Wb[y0:y0 + SIZE, x0:x0 + SIZE].cpu().numpy()
        assert rel_err(wgot[..., :5], Wo[halo:halo + SIZE, halo:halo + SIZE, :5]) < 2e-5, (y0, x0)
    # every pixel was written: the weight sums carry the 0.001 bias plus the zero-offset weight 1
    assert float(Wb[..., 4].min()) >= 1.0
    del Wb, out, out2


def test_pack_unpack_beyond_4_gib(ctx, huge, ts):
    s = ts.cuda_stream
    n = H * W * 4
    u8 = torch.empty((H, W, 4), device=huge.device, dtype=torch.uint8)
    assert mid.lib.mid_pack_u8(ctx.handle, huge.data_ptr(), n, u8.data_ptr(), s) == 0
    back = torch.empty_like(huge)
    assert mid.lib.mid_unpack_u8(ctx.handle, u8.data_ptr(), n, 0, back.data_ptr(), s) == 0
    torch.cuda.synchronize()
    for rows in (slice(0, 64), slice(8184 - 32, 8184 + 32), slice(H - 64, H)):
        h = huge[rows].cpu().numpy()
        assert np.array_equal(u8[rows].cpu().numpy(), oracle.pack_u8(h))
        assert np.array_equal(back[rows].cpu().numpy(), oracle.unpack_u8(oracle.pack_u8(h)))
    # whole buffer, on the device: pack(unpack(pack(x))) == pack(x)  (codes are fixed points of decode -> encode? not for
    # every code under truncation -- so the property checked is the weaker, exact one: the round trip never moves UP and
    # loses at most one code)
    u8b = torch.empty_like(u8)
    assert mid.lib.mid_pack_u8(ctx.handle, back.data_ptr(), n, u8b.data_ptr(), s) == 0
    torch.cuda.synchronize()
    d = u8.to(torch.int16) - u8b.to(torch.int16)
    assert int(d.min()) >= 0 and int(d.max()) <= 1
    del u8, u8b, back, d


# ---- layer-guided NLM: guides of 1.1 GB each, the same index arithmetic on 4-byte texels ----------------------------------------
def _guide(ts, i, seed, jitter=3):
    """RGBA8 guide i on the device: test_gpu_nlm_layers.guides' pattern (smooth in x and y, +-jitter codes of noise), so that at
    h = 0.5 many weights are neither 0 nor 1.  Built in row blocks: no temporary larger than the guide itself."""
    dev = torch.device("cuda", 0)
    with torch.cuda.stream(ts):
        gen = torch.Generator(device=dev).manual_seed(seed)
        out = torch.empty((H, W, 4), device=dev, dtype=torch.uint8)
        xx = torch.arange(W, device=dev, dtype=torch.int32)[None, :]
        for y0 in range(0, H, 2048):
            yy = torch.arange(y0, min(y0 + 2048, H), device=dev, dtype=torch.int32)[:, None]
            g = torch.stack([(xx * (1 + i)) % 256 + 0 * yy, (yy * 2 + 7 * i) % 256 + 0 * xx, (xx + yy) // 2 % 256,
                             torch.full((yy.shape[0], W), 255, device=dev, dtype=torch.int32)], -1)
            g = g + torch.randint(-jitter, jitter + 1, g.shape, device=dev, generator=gen, dtype=torch.int32)
            out[y0:y0 + yy.shape[0]] = g.clamp_(0, 255).to(torch.uint8)
            del g
    ts.synchronize()
    return out


def _crop_u8(g_dev, y0, x0, halo):
    """_crop for the uint8 guides: window + halo, zero beyond the frame."""
    ya, yb, xa, xb = y0 - halo, y0 + SIZE + halo, x0 - halo, x0 + SIZE + halo
    out = np.zeros((yb - ya, xb - xa, 4), np.uint8)
    sy, sx = slice(max(ya, 0), min(yb, H)), slice(max(xa, 0), min(xb, W))
    out[sy.start - ya:sy.stop - ya, sx.start - xa:sx.stop - xa] = g_dev[sy, sx].cpu().numpy()
    return out


def _window(t, y0, x0):
    return t[y0:y0 + SIZE, x0:x0 + SIZE].cpu().numpy()


def _nlm_layers_fused_and_chain(ctx, huge, ts, search, patch):
    """mid_nlm_layers with two guides against the checker on crops, and against mid_nlm_layers_accum x 2 into a zeroed 8.6 GB W +
    mid_normalize bit for bit; returns the worst rel err."""
    s = ts.cuda_stream
    halo = max(-search[0], search[1] - 1) + max(-patch[0], patch[1] - 1)
    gl = [_guide(ts, i, 91 + i) for i in range(2)]
    assert gl[0].numel() > 2 ** 30
    out = torch.empty_like(huge)
    p = mid.NlmParams(W, H, 0.5, search[0], search[1], patch[0], patch[1], mid.FMT_RGBA32F)
    tbl = (ctypes.c_void_p * 2)(*[g.data_ptr() for g in gl])
    assert mid.lib.mid_nlm_layers(ctx.handle, ctypes.byref(p), huge.data_ptr(), tbl, 2, out.data_ptr(), s) == 0, mid.lib.mid_last_error()
    with torch.cuda.stream(ts):
        Wb = torch.zeros((H, W, 8), device=huge.device, dtype=torch.float32)
    assert Wb.numel() * 4 > 2 ** 33
    out2 = torch.empty_like(huge)
    for g in gl:
        assert mid.lib.mid_nlm_layers_accum(ctx.handle, ctypes.byref(p), huge.data_ptr(), g.data_ptr(), Wb.data_ptr(), s) == 0, mid.lib.mid_last_error()
    q = mid.NormalizeParams(W, H)
    assert mid.lib.mid_normalize(ctx.handle, ctypes.byref(q), Wb.data_ptr(), out2.data_ptr(), s) == 0, mid.lib.mid_last_error()
    torch.cuda.synchronize()
    worst = 0.0
    for y0, x0 in WINDOWS:
        ref = np_nlm_layers.nlm_layers(_crop(huge, y0, x0, halo), [_crop_u8(g, y0, x0, halo) for g in gl], 0.5, search, patch)
        a = _window(out, y0, x0)
        e = rel_err(a, ref[halo:halo + SIZE, halo:halo + SIZE])
        worst = max(worst, e)
        assert e < TOL, (y0, x0, e)
        assert np.array_equal(a.view(np.uint32), _window(out2, y0, x0).view(np.uint32)), ("fused == accumulate x 2 + normalize", y0, x0)
    # every pixel was written by both dispatches: per layer the 0.001 bias plus the zero-offset weight 1
    assert float(Wb[..., 4].min()) >= 2.0
    del Wb, out, out2, gl
    torch.cuda.empty_cache()
    return worst


def test_nlm_layers_strip_kernel_beyond_4_gib(ctx, huge, ts):
    e = _nlm_layers_fused_and_chain(ctx, huge, ts, (-10, 11), (-3, 4))
    print(f"16400 x 16400, two guides, 21x21 / 7x7 (strip kernel): worst rel err over the windows {e:.2e}")


def test_nlm_layers_per_pixel_kernel_beyond_4_gib(ctx, huge, ts):
    e = _nlm_layers_fused_and_chain(ctx, huge, ts, (-2, 3), (-1, 2))
    print(f"16400 x 16400, two guides, 5x5 / 3x3 (per-pixel kernel): worst rel err over the windows {e:.2e}")


def test_nlm_layers_temporal_beyond_4_gib(ctx, huge, ts):
    # two huge frames, k = 1, one guide each: both outputs against the checker on crops, and against the chain of
    # mid_nlm_layers_pair_accum dispatches (neighbours ascending) + mid_normalize bit for bit
    search, patch, halo = (-10, 11), (-3, 4), 13
    s = ts.cuda_stream
    dev = huge.device
    with torch.cuda.stream(ts):
        gen = torch.Generator(device=dev).manual_seed(93)
        second = torch.rand((H, W, 4), device=dev, generator=gen, dtype=torch.float32)
    frames = [huge, second]
    gl = [_guide(ts, 0, 94), _guide(ts, 0, 95)]          # one scene, the guides a few codes apart from frame to frame
    outs = [torch.empty_like(huge) for _ in range(2)]
    p = mid.NlmParams(W, H, 0.5, search[0], search[1], patch[0], patch[1], mid.FMT_RGBA32F)
    assert mid.lib.mid_nlm_layers_temporal(ctx.handle, ctypes.byref(p), (ctypes.c_void_p * 2)(*[f.data_ptr() for f in frames]),
                                           (ctypes.c_void_p * 2)(*[g.data_ptr() for g in gl]), 1, 2, 1, 0, 2,
                                           (ctypes.c_void_p * 2)(*[o.data_ptr() for o in outs]), mid.FMT_RGBA32F, s) == 0, mid.lib.mid_last_error()
    torch.cuda.synchronize()
    worst = 0.0
    for y0, x0 in WINDOWS:
        ref = np_nlm_layers_temporal.nlm_layers_temporal([_crop(f, y0, x0, halo) for f in frames],
                                                         [[_crop_u8(g, y0, x0, halo)] for g in gl], 1, 0.5, search, patch)
        for t in range(2):
            e = rel_err(_window(outs[t], y0, x0), ref[t][halo:halo + SIZE, halo:halo + SIZE])
            worst = max(worst, e)
            assert e < TOL, (t, y0, x0, e)
    print(f"16400 x 16400, two frames, k = 1, one guide each, 21x21 / 7x7: worst rel err over the windows {worst:.2e}")
    with torch.cuda.stream(ts):
        Wb = torch.empty((H, W, 8), device=dev, dtype=torch.float32)
    out2 = torch.empty_like(huge)
    q = mid.NormalizeParams(W, H)
    for t in range(2):
        with torch.cuda.stream(ts):
            Wb.zero_()
        for f in range(2):
            assert mid.lib.mid_nlm_layers_pair_accum(ctx.handle, ctypes.byref(p), gl[t].data_ptr(), gl[f].data_ptr(), frames[f].data_ptr(),
                                                     Wb.data_ptr(), s) == 0, mid.lib.mid_last_error()
        assert mid.lib.mid_normalize(ctx.handle, ctypes.byref(q), Wb.data_ptr(), out2.data_ptr(), s) == 0, mid.lib.mid_last_error()
        torch.cuda.synchronize()
        for y0, x0 in WINDOWS:
            assert np.array_equal(_window(outs[t], y0, x0).view(np.uint32), _window(out2, y0, x0).view(np.uint32)), (t, y0, x0)
        # every pixel was written: the dispatch of frame t with itself has the zero-offset weight 1 (the other frame's guide differs)
        assert float(Wb[..., 4].min()) >= 1.0
    del Wb, out2, outs, gl, second, frames
    torch.cuda.empty_cache()


def test_nlm_joint_strip_kernel_beyond_4_gib(ctx, huge, ts):
    # two guides with unequal h on the 21x21 / 7x7 window: the class of eight waves of four rows on 32-row tiles, 513 x 283 of them.
    # The output holds NaN before the call, so a tile the remap of the tile index leaves out shows in the scan of the whole buffer.
    search, patch, halo, hs = (-10, 11), (-3, 4), 13, (0.5, 0.8)
    s = ts.cuda_stream
    gl = [_guide(ts, i, 96 + i) for i in range(2)]
    assert gl[0].numel() > 2 ** 30
    with torch.cuda.stream(ts):
        out = torch.full_like(huge, float("nan"))
    p = mid.NlmParams(W, H, 0.5, search[0], search[1], patch[0], patch[1], mid.FMT_RGBA32F)
    assert mid.lib.mid_nlm_joint(ctx.handle, ctypes.byref(p), (ctypes.c_float * 2)(*hs), (ctypes.c_void_p * 1)(huge.data_ptr()),
                                 (ctypes.c_void_p * 2)(*[g.data_ptr() for g in gl]), 2, 1, 0, 0, 1, (ctypes.c_void_p * 1)(out.data_ptr()),
                                 mid.FMT_RGBA32F, s) == 0, mid.lib.mid_last_error()
    torch.cuda.synchronize()
    worst = 0.0
    for y0, x0 in WINDOWS:
        ref = np_nlm_joint.nlm_joint([_crop(huge, y0, x0, halo)], [[_crop_u8(g, y0, x0, halo) for g in gl]], hs, 0, search, patch)[0]
        e = rel_err(_window(out, y0, x0), ref[halo:halo + SIZE, halo:halo + SIZE])
        worst = max(worst, e)
        assert e < TOL, (y0, x0, e)
    print(f"16400 x 16400, joint NLM, two guides, h = {hs}, 21x21 / 7x7 (32-row strip kernel): worst rel err over the windows {worst:.2e}")
    assert not torch.isnan(out).any(), "every tile was dealt"
    del out, gl
    torch.cuda.empty_cache()
