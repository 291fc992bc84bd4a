"""GPU suite: what mid_guided_filter (section a4o) touches and what it refuses.

`out` and `work` between guard bands (work at exactly the size the workspace query returns), the inputs inside NaN bytes; outputs that
hold NaN before the call: every pixel written; NaN / +-Inf planted on corners, edges and every seam, in `in`, in `guide` and in both;
a frame with nothing valid; a 262149 x 1 strip and a 1 x 70000 column at radius 16; every refusal of the header, `out` untouched."""
import ctypes

import numpy as np
import pytest
import torch

import image_denoising_filter_amd as mid
import guided_inputs as gi
import np_guided

pytestmark = pytest.mark.gpu
FMT = {np.dtype(np.float32): mid.FMT_RGBA32F, np.dtype(np.uint8): mid.FMT_RGBA8, np.dtype(np.float16): mid.FMT_RGBA16F}
GUARD = 0xFF          # as a float, a half or four of them: NaN


def guarded(nbytes, fill_from=None, band=8192):
    """A device buffer of nbytes inside `band` bytes of 0xFF on either side (and 0xFF inside, unless fill_from gives its content)."""
    raw = torch.full((nbytes + 2 * band,), GUARD, dtype=torch.uint8, device="cuda:0")
    if fill_from is not None:
        raw[band:band + nbytes] = torch.from_numpy(np.ascontiguousarray(fill_from).view(np.uint8).reshape(-1)).to("cuda:0")
    return raw, raw.data_ptr() + band


def call(ctx, frame, guide, radius, eps, out_dt=np.float32):
    """The C entry point on guarded buffers; asserts the bands and the inputs intact and returns the output."""
    h, w = frame.shape[:2]
    out_dt = np.dtype(out_dt)
    p = mid.GuidedParams(w, h, radius, eps, mid.api.fmt_with_guide(FMT[frame.dtype], FMT[(frame if guide is None else guide).dtype]))
    n = ctypes.c_size_t()
    assert mid.lib.mid_guided_workspace(ctypes.byref(p), ctypes.byref(n)) == 0
    assert n.value == 52 * h * w                                    # the header: 52 bytes per pixel and no constant
    band = 64 * w * 16 + 8192
    band -= band % 16
    n_out = h * w * 4 * out_dt.itemsize
    r_in, p_in = guarded(frame.nbytes, frame, band)
    r_g, p_g = (None, None) if guide is None else guarded(guide.nbytes, guide, band)
    r_work, p_work = guarded(n.value, None, band)
    r_out, p_out = guarded(n_out, None, band)
    torch.cuda.synchronize()
    rc = mid.lib.mid_guided_filter(ctx.handle, ctypes.byref(p), p_in, p_g, p_work, p_out, FMT[out_dt], None)
    assert rc == 0, mid.lib.mid_last_error()
    ctx.sync()
    for raw, nb, name in ((r_work, n.value, "work"), (r_out, n_out, "out")):
        assert bool((raw[:band] == GUARD).all()) and bool((raw[band + nb:] == GUARD).all()), f"the bands around {name}"
    for raw, x in ((r_in, frame), (r_g, guide)):
        if x is not None:
            assert bool((raw[:band] == GUARD).all()) and bool((raw[band + x.nbytes:] == GUARD).all())
            assert np.array_equal(raw[band:band + x.nbytes].cpu().numpy(), x.view(np.uint8).reshape(-1))
    return r_out[band:band + n_out].cpu().numpy().view(out_dt).reshape(h, w, 4).copy()


@pytest.mark.parametrize("shape", [(1, 1), (5, 5), (65, 225), (66, 257), (3, 513)], ids=lambda s: f"{s[1]}x{s[0]}")
@pytest.mark.parametrize("radius", (1, 16))
def test_guard_bands_and_every_pixel_written(ctx, shape, radius):
    h, w = shape
    noisy, alb, _ = gi.scene(h, w, radius)
    for frame, guide, out_dt in ((noisy, alb, np.float32), (gi.as_dtype(noisy, np.uint8), gi.as_dtype(alb, np.float16), np.float16),
                                 (noisy, None, np.uint8)):
        got = call(ctx, frame, guide, radius, gi.EPS, out_dt)
        ref = np_guided.guided(frame, guide, radius, gi.EPS)
        if out_dt == np.float32:
            assert np.isfinite(got).all()                               # `out` held NaN before the call: every pixel was written
            assert np_guided.worst_share(got, ref) <= 1.0
        elif out_dt == np.float16:
            assert np.isfinite(got.astype(np.float32)).all()
            # binary16 of the float output: half an ulp of a normal half (2^-11 relative), or of a subnormal one (2^-25)
            slack = np_guided.tolerance(ref) + 2.0 ** -11 * (np.abs(ref["out"][..., :3]) + np_guided.tolerance(ref)) + 2.0 ** -25
            assert (np.abs(got[..., :3].astype(np.float64) - ref["out"][..., :3]) <= slack).all()
        else:
            # (0xFF bytes are a legal u8 texel: the float32 call above has shown every pixel written; here the values)
            # mid_pack_u8 truncates 255 v: within one level below the clipped value, plus the float output's own bound
            assert float(np.abs(got.astype(np.float64) / 255 - np.clip(ref["out"], 0, 1)).max()) <= 1 / 255 + float(np_guided.tolerance(ref).max())


def plant(h, w, radius, where):
    noisy, alb, _ = gi.scene(h, w, radius)
    alb = alb.copy()
    sw = gi.strip_w(radius)
    xs = sorted({x for x in (0, w - 1, w // 2, 63, 64, sw - 1, sw, 255, 256) if 0 <= x < w})
    P = gi.PERIOD
    ys = sorted({y for y in (0, h - 1, h // 2, P - 1, P, P + radius, P - radius, 2 * P - 1, 2 * P) if 0 <= y < h})
    spots = [(y, x) for y in ys for x in xs]
    for k, (y, x) in enumerate(spots):
        bad = (np.nan, np.inf, -np.inf)[k % 3]
        if where in ("in", "both"):
            noisy[y, x, k % 3] = bad
        if where in ("guide", "both"):
            alb[y, x, (k + 1) % 3] = bad
    noisy[h // 3, w // 3, 3] = np.nan                                   # a non-finite ALPHA does not count (and comes back)
    alb[h // 3, w // 4, 3] = np.inf
    return noisy, alb, spots


@pytest.mark.parametrize("where", ("in", "guide", "both"))
@pytest.mark.parametrize("radius", (1, 3, 16))
def test_non_finite_texels_on_corners_edges_and_seams(ctx, where, radius):
    h, w = 70, 261
    noisy, alb, spots = plant(h, w, radius, where)
    ref = np_guided.guided(noisy, alb, radius, gi.EPS)
    assert int((~ref["valid"]).sum()) == len(spots)      # (at radius 1 the planted seams x = 253 .. 256 leave windows without a model)
    got = call(ctx, noisy, alb, radius, gi.EPS)
    assert np_guided.worst_share(got, ref) <= 1.0                       # (which also compares the passed-through texels exactly)
    assert np.isfinite(got[ref["filtered"]][..., :3]).all()
    if where == "in":                                                   # the frame guiding itself through the same holes
        ref = np_guided.guided(noisy, None, radius, gi.EPS)
        assert np_guided.worst_share(call(ctx, noisy, None, radius, gi.EPS), ref) <= 1.0


def test_a_hole_larger_than_the_window_and_nothing_valid(ctx):
    h, w, radius = 70, 130, 2
    noisy, alb, _ = gi.scene(h, w, radius)
    alb = alb.copy()
    alb[20:40, 50:80, 0] = np.nan                                       # windows without a model, pixels with m = 0
    ref = np_guided.guided(noisy, alb, radius, gi.EPS)
    assert (~ref["model"]).sum() == 16 * 26
    assert np_guided.worst_share(call(ctx, noisy, alb, radius, gi.EPS), ref) <= 1.0
    noisy[..., 1] = np.nan
    got = call(ctx, noisy, alb, radius, gi.EPS)
    assert got.tobytes() == noisy.tobytes()


@pytest.mark.parametrize("shape", [(1, 262149), (70000, 1)], ids=["262149x1", "1x70000"])
def test_long_strips_at_radius_16(ctx, shape):
    h, w = shape
    radius = 16
    rng = np.random.default_rng(h + w)
    n = h * w
    # blocks of 64 along the long axis, noise on top: the recipe's shape in one dimension
    alb = (0.15 + 0.8 * rng.random((n // 64 + 1, 3))).repeat(64, 0)[:n]
    frame = np.ones((n, 4), np.float32)
    guide = np.ones((n, 4), np.float32)
    guide[:, :3] = alb
    frame[:, :3] = alb * rng.gamma(4.0, 0.25, (n, 3))
    frame[n // 3, 0] = np.nan
    frame, guide = frame.reshape(h, w, 4), guide.reshape(h, w, 4)
    ref = np_guided.guided(frame, guide, radius, gi.EPS)
    got = call(ctx, frame, guide, radius, gi.EPS)
    share = np_guided.worst_share(got, ref)
    print(f"{w}x{h}: worst error {share:.3f} of the tolerance")
    assert share <= 1.0


def test_refusals_leave_out_and_work_untouched(ctx):
    h, w, radius = 20, 70, 2
    noisy, alb, _ = gi.scene(h, w, radius)
    g8 = gi.as_dtype(alb, np.uint8)
    d_in, d_g, d_g8 = ctx.upload(noisy), ctx.upload(alb), ctx.upload(g8)
    n_work, n_out = 52 * h * w, 16 * h * w
    work = torch.full((n_work + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    out = torch.full((n_out + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    both = torch.full((n_work + n_out,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    Wp, Op = work.data_ptr(), out.data_ptr()
    assert Wp % 16 == 0 and Op % 16 == 0
    F = mid.FMT_RGBA32F
    FF = mid.api.fmt_with_guide(F, F)
    good = dict(width=w, height=h, radius=radius, eps=1e-2, format=FF)

    def refused(word, ctx_h=ctx.handle, params=True, a=d_in.ptr, g=d_g.ptr, work=Wp, out=Op, out_fmt=F, **kw):
        p = mid.GuidedParams(**{**good, **kw})
        rc = mid.lib.mid_guided_filter(ctx_h, ctypes.byref(p) if params else None, a, g, work, out, out_fmt, None)
        assert rc == 1, (word, kw, rc)                                          # MID_ERR_INVALID
        msg = mid.lib.mid_last_error().decode()
        assert word in msg, (word, msg)

    refused("params is NULL", params=False)
    refused("NULL pointer", a=None)
    refused("NULL pointer", work=None)
    refused("NULL pointer", out=None)
    for r in (0, -1, 17, 1 << 20):
        refused("radius", radius=r)
    for v in (0.0, -1.0, float("nan"), float("inf")):
        refused("eps", eps=v)
    for kw in (dict(width=0), dict(height=0), dict(width=-3)):
        refused("bad size", **kw)
    refused("too large", width=1 << 15, height=1 << 15)
    refused("unknown format", format=3)
    refused("unknown format", format=mid.api.fmt_with_guide(F, 5))
    refused("unknown format", format=FF | (1 << 16))
    refused("unknown out_format", out_fmt=3)
    refused("in is not 16-byte aligned", a=d_in.ptr + 8)
    refused("guide is not 16-byte aligned", g=d_g.ptr + 4)
    refused("guide is not 4-byte aligned", g=d_g8.ptr + 2, format=F)
    refused("in is not 8-byte aligned", a=d_in.ptr + 4, format=mid.api.fmt_with_guide(mid.FMT_RGBA16F, F))
    refused("out is not 16-byte aligned", out=Op + 8)
    refused("out is not 8-byte aligned", out=Op + 4, out_fmt=mid.FMT_RGBA16F)
    refused("out is not 4-byte aligned", out=Op + 2, out_fmt=mid.FMT_RGBA8)
    refused("work is not 16-byte aligned", work=Wp + 8)
    refused("out overlaps an input", out=d_in.ptr)                              # exactly in place
    refused("out overlaps an input", out=d_in.ptr + 16 * (h * w - 1))
    refused("out overlaps an input", out=d_g.ptr)
    refused("work overlaps an input", work=d_in.ptr)
    refused("work overlaps an input", work=d_g.ptr + 16 * (h * w - 1))
    refused("out overlaps work", work=both.data_ptr(), out=both.data_ptr() + n_work - 16)
    refused("out overlaps work", work=both.data_ptr() + n_out - 16, out=both.data_ptr())
    refused("names another guide format", g=d_in.ptr, format=F)                 # guide == in, but the word says RGBA8 guides
    # the workspace query refuses the same parameters, and a NULL `bytes`
    n = ctypes.c_size_t(12345)
    assert mid.lib.mid_guided_workspace(ctypes.byref(mid.GuidedParams(**good)), None) == 1
    assert mid.lib.mid_guided_workspace(None, ctypes.byref(n)) == 1
    assert mid.lib.mid_guided_workspace(ctypes.byref(mid.GuidedParams(**{**good, "radius": 17})), ctypes.byref(n)) == 1 and n.value == 12345
    ctx.sync()
    torch.cuda.synchronize()
    for buf in (work, out, both):
        assert bool((buf == 0xA5).all())
    assert np.array_equal(ctx.download(d_in, noisy.shape, np.float32), noisy) and np.array_equal(ctx.download(d_g, alb.shape, np.float32), alb)
    # and what is allowed: guide == in with the frame's format, out right behind work
    p = mid.GuidedParams(**good)
    assert mid.lib.mid_guided_filter(ctx.handle, ctypes.byref(p), d_in.ptr, d_in.ptr, both.data_ptr(), both.data_ptr() + n_work, F, None) == 0, mid.lib.mid_last_error()
    ctx.sync()
    got = both[n_work:].cpu().numpy().view(np.float32).reshape(h, w, 4)
    assert np_guided.worst_share(got, np_guided.guided(noisy, None, radius, 1e-2)) <= 1.0
