"""GPU suite: the bit identities of mid_guided_filter (section a4o).

Repeated calls and a second stream give the same bits (no atomics, a grid that depends on the size alone); a u8 frame and a u8 guide
against their float32 widenings; `in` scaled by 2^+-k scales `out` by it (every operation is linear in p and a power of two commutes
with every rounding while nothing leaves the normal range); guide == NULL and guide == in; an invalid pixel comes back as its input
texel; out.a == in.a everywhere."""
import ctypes

import numpy as np
import pytest
import torch

import image_denoising_filter_amd as mid
import guided_inputs as gi
import np_guided

pytestmark = pytest.mark.gpu
H, W = 67, 259


def raw_call(ctx, frame, guide, radius, eps, stream=None, same_pointer=False):
    h, w = frame.shape[:2]
    fi = mid.api._fmt_of(frame)
    fg = fi if guide is None else mid.api._fmt_of(guide)
    p = mid.GuidedParams(w, h, radius, eps, mid.api.fmt_with_guide(fi, fg))
    n = ctypes.c_size_t()
    assert mid.lib.mid_guided_workspace(ctypes.byref(p), ctypes.byref(n)) == 0
    d_in, d_work, d_out = ctx.upload(frame), ctx.alloc(n.value), ctx.alloc(h * w * 16)
    d_g = None if guide is None else ctx.upload(guide)
    g_ptr = d_in.ptr if same_pointer else None if d_g is None else d_g.ptr
    ctx.sync()
    torch.cuda.synchronize()
    rc = mid.lib.mid_guided_filter(ctx.handle, ctypes.byref(p), d_in.ptr, g_ptr, d_work.ptr, d_out.ptr, mid.FMT_RGBA32F, stream)
    assert rc == 0, mid.lib.mid_last_error()
    if stream is not None:
        torch.cuda.synchronize()
    return ctx.download(d_out, (h, w, 4), np.float32)


@pytest.mark.parametrize("radius", (2, 16))
def test_repeated_calls_and_a_second_stream(ctx, radius):
    noisy, alb, _ = gi.scene(H, W, radius)
    first = raw_call(ctx, noisy, alb, radius, gi.EPS)
    assert raw_call(ctx, noisy, alb, radius, gi.EPS).tobytes() == first.tobytes()
    s = torch.cuda.Stream(device="cuda:0")
    assert raw_call(ctx, noisy, alb, radius, gi.EPS, stream=ctypes.c_void_p(s.cuda_stream)).tobytes() == first.tobytes()


@pytest.mark.parametrize("radius", (1, 8))
def test_u8_against_its_float32_widening(ctx, radius):
    noisy, alb, _ = gi.scene(H, W, radius)
    f8, g8 = gi.as_dtype(noisy, np.uint8), gi.as_dtype(alb, np.uint8)
    wide = lambda x: (x.astype(np.float32) / np.float32(255)).astype(np.float32)
    got = ctx.guided_filter(f8, g8, radius, gi.EPS)
    assert got.tobytes() == ctx.guided_filter(wide(f8), wide(g8), radius, gi.EPS).tobytes()
    assert got.tobytes() == ctx.guided_filter(f8, wide(g8), radius, gi.EPS).tobytes()


@pytest.mark.parametrize("k", (-6, -1, 3, 10))
def test_scaling_the_frame_by_a_power_of_two(ctx, k):
    radius = 3
    noisy, alb, _ = gi.scene(H, W, radius)
    s = np.float32(2.0 ** k)
    scaled = noisy.copy()
    scaled[..., :3] *= s
    base, got = ctx.guided_filter(noisy, alb, radius, gi.EPS), ctx.guided_filter(scaled, alb, radius, gi.EPS)
    want = base.copy()
    want[..., :3] *= s
    tiny = np.abs(want[..., :3]) < 2.0 ** -100          # (nothing here: the identity holds while no value leaves the normal range)
    assert not tiny.any() or k > 0
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("dt", (np.uint8, np.float16, np.float32), ids=lambda d: np.dtype(d).name)
def test_null_guide_and_guide_equal_to_in(ctx, dt):
    radius = 2
    frame = gi.as_dtype(gi.scene(H, W, radius)[0], dt)
    a = raw_call(ctx, frame, None, radius, gi.EPS)
    b = raw_call(ctx, frame, None, radius, gi.EPS, same_pointer=True)
    c = raw_call(ctx, frame, frame.copy(), radius, gi.EPS)      # and a second copy of the frame as the guide
    assert a.tobytes() == b.tobytes() == c.tobytes()


def test_invalid_pixels_and_alpha_come_back_bit_for_bit(ctx):
    radius = 2
    noisy, alb, _ = gi.scene(H, W, radius)
    alb = alb.copy()
    rng = np.random.default_rng(5)
    bits = noisy.view(np.uint32)
    spots = [(0, 0), (H - 1, W - 1), (63, 251), (64, 252), (10, 64)]
    for i, (y, x) in enumerate(spots):
        if i % 2:
            alb[y, x, i % 3] = (np.nan, np.inf, -np.inf)[i % 3]     # invalid through the guide: the frame's texel is finite
        else:
            bits[y, x, i % 3] = (0x7FC12345, 0x7F800000, 0xFF800000)[i % 3]     # a NaN with a payload, +Inf, -Inf
    bits[..., 3] = rng.integers(0, 2 ** 32, (H, W), dtype=np.uint64).astype(np.uint32)      # alpha: any bits at all, NaNs among them
    ref = np_guided.guided(noisy, alb, radius, gi.EPS)
    got = ctx.guided_filter(noisy, alb, radius, gi.EPS)
    for y, x in spots:
        assert not ref["filtered"][y, x]
        assert got.view(np.uint32)[y, x].tobytes() == bits[y, x].tobytes()
    assert np.array_equal(got.view(np.uint32)[..., 3], bits[..., 3])
    f = ref["filtered"]
    err = np.abs(got[f][..., :3].astype(np.float64) - ref["out"][f][..., :3])
    assert float((err / np_guided.tolerance(ref)[f]).max()) <= 1.0
