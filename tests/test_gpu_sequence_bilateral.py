"""GPU suite: mid_sequence_bilateral -- a whole animation through the frame pipeline with the bilateral (plain, or guided by each
frame's own layers) as its compute stage.

Every comparison is on raw bits against per-frame device calls (ctx.bilateral / ctx.bilateral_layers, then ctx.pack_u8 /
ctx.pack_f16 for packed outputs), which the existing suites pin to the oracle and the reference fixtures."""
import ctypes

import numpy as np
import pytest

import image_denoising_filter_amd as mid
from conftest import synth_hdr

pytestmark = pytest.mark.gpu

SS, SC = 2.0, 0.2
DT = {"f32": np.float32, "u8": np.uint8, "f16": np.float16}


def frames_of(rng, n, h, w, dt):
    out = []
    for _ in range(n):
        f = (synth_hdr(rng, h, w, 1.0) * 0.3).astype(np.float32)
        f[..., 3] = 1.0
        if rng.random() < 0.5:
            f[rng.random((h, w)) < 0.02, 3] = 0.5          # some translucent texels: the tiled kernels' non-opaque branch
        if dt == np.uint8:
            out.append(np.clip(f * 255, 0, 255).astype(np.uint8))
        else:
            out.append(f.astype(dt))
    return out


def layers_of(rng, n, L, h, w):
    return [[rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(L)] for _ in range(n)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def packed(ctx, ref, out_dt):
    if out_dt == np.uint8:
        return ctx.pack_u8(ref)
    if out_dt == np.float16:
        return ctx.pack_f16(ref)
    return ref


def want_plain(ctx, frames, r, layout, out_dt):
    return [packed(ctx, ctx.bilateral(f, r, SS, SC, layout), out_dt) for f in frames]


def want_layers(ctx, frames, layers, r, out_dt):
    return [packed(ctx, ctx.bilateral_layers(f, ls, r, SS, SC), out_dt) for f, ls in zip(frames, layers)]


def assert_same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (i, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), f"output {i} differs"


def _direct(ctx):
    _, outs = ctx.pipe_last_timeline()
    return all(ds == ke and de == ke for _, _, ke, ds, de in outs)


@pytest.mark.parametrize("layout", ["texture", "linear"])
@pytest.mark.parametrize("r", [4, 8, 20, 13])
def test_plain_every_format_pair(ctx, r, layout):
    rng = np.random.default_rng(100 + r)
    h, w, n = 45, 77, 6                                              # ragged; more frames than the 4-slot ring
    for in_name, in_dt in DT.items():
        frames = frames_of(rng, n, h, w, in_dt)
        ref = [ctx.bilateral(f, r, SS, SC, layout) for f in frames]
        for out_dt in DT.values():
            got, t = ctx.sequence_bilateral(frames, r, SS, SC, layout, out_dtype=out_dt)
            assert_same(got, [packed(ctx, x, out_dt) for x in ref])
            assert t[0] > 0 and t[1] > 0


@pytest.mark.parametrize("in_dt", [np.float32, np.uint8, np.float16])
def test_pinned_pageable_and_overlap(ctx, in_dt):
    rng = np.random.default_rng(7)
    h, w, n = 70, 130, 7
    frames = frames_of(rng, n, h, w, in_dt)
    layers = layers_of(rng, n, 2, h, w)
    for out_dt in DT.values():
        wp = want_plain(ctx, frames, 8, "texture", out_dt)
        wl = want_layers(ctx, frames, layers, 8, out_dt)
        for pinned in (True, False):
            for pinned_out in (True, False):
                for overlap in (True, False):
                    kw = dict(overlap=overlap, pinned=pinned, pinned_out=pinned_out, out_dtype=out_dt)
                    got, _ = ctx.sequence_bilateral(frames, 8, SS, SC, "texture", **kw)
                    assert_same(got, wp)
                    got, _ = ctx.sequence_bilateral(frames, 8, SS, SC, "texture", layers=layers, **kw)
                    assert_same(got, wl)


def test_one_frame_and_odd_sizes(ctx):
    rng = np.random.default_rng(3)
    for (h, w, n) in ((17, 33, 1), (1, 5, 2), (129, 65, 5)):
        for layout in ("texture", "linear"):
            frames = frames_of(rng, n, h, w, np.float32)
            for out_dt in DT.values():
                got, _ = ctx.sequence_bilateral(frames, 8, SS, SC, layout, out_dtype=out_dt)
                assert_same(got, want_plain(ctx, frames, 8, layout, out_dt))


@pytest.mark.parametrize("L", [1, 4, 16])
def test_layers_match_per_frame_calls(ctx, L):
    rng = np.random.default_rng(50 + L)
    h, w, n = 45, 77, 5
    outs = list(DT.values())
    for j, r in enumerate((8, 20, 13, 22, 24)):                      # tuned, tuned, run-time radius, generic kernel (22 and the largest, 24)
        in_dt = list(DT.values())[j % 3]
        out_dt = outs[(j + L) % 3]
        frames = frames_of(rng, n, h, w, in_dt)
        layers = layers_of(rng, n, L, h, w)
        got, _ = ctx.sequence_bilateral(frames, r, SS, SC, layers=layers, out_dtype=out_dt)
        assert_same(got, want_layers(ctx, frames, layers, r, out_dt))


def test_no_layers_gives_the_magenta_sentinel(ctx):
    rng = np.random.default_rng(4)
    frames = frames_of(rng, 3, 20, 70, np.float32)
    got, _ = ctx.sequence_bilateral(frames, 8, SS, SC, layers=[[], [], []])
    for g in got:
        assert np.array_equal(g, np.broadcast_to(np.float32([1, 0, 1, 1]), g.shape))
    got, _ = ctx.sequence_bilateral(frames, 8, SS, SC, layers=[[], [], []], out_dtype=np.uint8)
    for g in got:
        assert np.array_equal(g, np.broadcast_to(np.uint8([255, 0, 255, 255]), g.shape))


def test_each_output_uses_its_own_frames_layers(ctx):
    rng = np.random.default_rng(12)
    h, w, n = 40, 90, 6
    frames = frames_of(rng, n, h, w, np.float32)
    layers = layers_of(rng, n, 3, h, w)
    got, _ = ctx.sequence_bilateral(frames, 8, SS, SC, layers=layers)
    perm = [1, 0, 3, 2, 5, 4]
    swapped = [layers[p] for p in perm]
    got2, _ = ctx.sequence_bilateral(frames, 8, SS, SC, layers=swapped)
    assert_same(got2, want_layers(ctx, frames, swapped, 8, np.float32))
    for i in range(n):
        assert not np.array_equal(got[i], got2[i]), f"output {i} did not change when its layers did"


@pytest.mark.parametrize("layered", [False, True])
def test_direct_stores_for_packed_outputs_in_one_allocation(ctx, layered):
    rng = np.random.default_rng(21)
    h, w, n = 64, 128, 6
    frames = frames_of(rng, n, h, w, np.float32)
    layers = layers_of(rng, n, 2, h, w) if layered else None
    for out_dt, direct in ((np.uint8, True), (np.float16, True), (np.float32, False)):
        got, _ = ctx.sequence_bilateral(frames, 8, SS, SC, layers=layers, out_dtype=out_dt)
        assert _direct(ctx) == direct, out_dt
        want = want_layers(ctx, frames, layers, 8, out_dt) if layered else want_plain(ctx, frames, 8, "texture", out_dt)
        assert_same(got, want)
    # pageable outputs are downloaded
    ctx.sequence_bilateral(frames, 8, SS, SC, layers=layers, out_dtype=np.uint8, pinned_out=False)
    assert not _direct(ctx)


@pytest.mark.parametrize("out_dt", [np.uint8, np.float16])
def test_output_spanning_two_registrations_is_staged_and_correct(ctx, out_dt):
    rng = np.random.default_rng(22)
    h, w = 64, 128
    F = h * w * 4 * np.dtype(out_dt).itemsize                           # one output frame, a page multiple
    frames = frames_of(rng, 2, h, w, np.float32)
    want = want_plain(ctx, frames, 8, "texture", out_dt)
    hin = [f.ctypes.data for f in frames]
    raw = np.zeros(4 * F + 4096, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 4096
    assert mid.lib.mid_host_register(ctx.handle, base, 2 * F) == 0
    try:
        assert mid.lib.mid_host_register(ctx.handle, base + 2 * F, 2 * F) == 0
        try:
            # output 0 inside the first registration, output 1 across the boundary of the two: neither is stored by the kernel
            outs = [base, base + 2 * F - F // 2]
            ctx.sequence_bilateral_pinned(hin, outs, w, h, mid.FMT_RGBA32F, 8, SS, SC, out_dtype=out_dt)
            assert not _direct(ctx)
            off = base - raw.ctypes.data
            for i, o in enumerate(outs):
                g = raw[o - base + off:o - base + off + F].view(out_dt).reshape(h, w, 4)
                assert np.array_equal(bits(g), bits(want[i])), i
        finally:
            assert mid.lib.mid_host_unregister(ctx.handle, base + 2 * F) == 0
    finally:
        assert mid.lib.mid_host_unregister(ctx.handle, base) == 0


def test_refusals_queue_no_work(ctx):
    rng = np.random.default_rng(30)
    h, w = 24, 40
    frames = frames_of(rng, 2, h, w, np.float32)
    lay = layers_of(rng, 2, 1, h, w)
    ctx.sequence_bilateral(frames, 8, SS, SC)                         # a completed call whose timeline a refusal must not replace
    before = ctx.pipe_last_timeline()
    outs = [np.full((h, w, 4), 0xAB, np.uint8) for _ in range(2)]
    P = ctypes.c_void_p

    def call(p=None, fr=None, n=2, lp=None, nl=0, ou=None, out_fmt=mid.FMT_RGBA8, nf=None):
        p = p or mid.BilateralParams(w, h, SS, SC, 8, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)
        fr = fr if fr is not None else [f.ctypes.data for f in frames]
        ou = ou if ou is not None else [o.ctypes.data for o in outs]
        tl = None if lp is None else (P * max(len(lp), 1))(*lp)
        return mid.lib.mid_sequence_bilateral(ctx.handle, ctypes.byref(p), (P * len(fr))(*fr), n if nf is None else nf, tl, nl,
                                              (P * len(ou))(*ou), out_fmt, 1, None)

    lp = [l[0].ctypes.data for l in lay]
    B = mid.BilateralParams
    cases = {
        "NULL frame": dict(fr=[frames[0].ctypes.data, None]),
        "NULL layer": dict(lp=[lp[0], None], nl=1),
        "NULL output": dict(ou=[outs[0].ctypes.data, None]),
        "17 layers": dict(lp=lp * 17, nl=17),
        "negative layers": dict(lp=lp, nl=-1),
        "layers + linear": dict(p=B(w, h, SS, SC, 8, mid.LAYOUT_LINEAR, mid.FMT_RGBA32F), lp=lp, nl=1),
        "unknown out_format": dict(out_fmt=5),
        "negative out_format": dict(out_fmt=-1),
        "output is a frame": dict(ou=[outs[0].ctypes.data, frames[0].ctypes.data]),
        "output is a layer": dict(ou=[lp[1], outs[1].ctypes.data], lp=lp, nl=1),
        "output twice": dict(ou=[outs[0].ctypes.data, outs[0].ctypes.data]),
        "radius 0": dict(p=B(w, h, SS, SC, 0, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)),
        "radius 25": dict(p=B(w, h, SS, SC, 25, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)),
        "sigma 0": dict(p=B(w, h, 0.0, SC, 8, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)),
        "bad size": dict(p=B(0, h, SS, SC, 8, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)),
        "unknown format": dict(p=B(w, h, SS, SC, 8, mid.LAYOUT_TEXTURE, 7)),
        "unknown layout": dict(p=B(w, h, SS, SC, 8, 2, mid.FMT_RGBA32F)),
        "no frames": dict(nf=0),
    }
    for what, kw in cases.items():
        assert call(**kw) == 1, what
        assert mid.lib.mid_last_error(), what
        assert all((o == 0xAB).all() for o in outs), what
        assert ctx.pipe_last_timeline() == before, what
    d_in, d_out = ctx.upload(frames[0]), ctx.alloc(h * w * 16)
    with ctx.record() as rec:                                       # a recording with one launch in it, then the refused call
        ctx.bilateral_dev(d_in.ptr, d_out.ptr, w, h, 8, SS, SC, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)
        rc = call()
    assert rec.info()[0] == 1
    rec.close()
    assert rc == 1 and b"recording" in mid.lib.mid_last_error()
    assert all((o == 0xAB).all() for o in outs)
    assert ctx.pipe_last_timeline() == before
    got, _ = ctx.sequence_bilateral(frames, 8, SS, SC, out_dtype=np.uint8)      # the context works on
    assert_same(got, want_plain(ctx, frames, 8, "texture", np.uint8))


def test_1080p_layers_u8(ctx):
    rng = np.random.default_rng(1080)
    h, w, n, L = 1080, 1920, 8, 4
    frames = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(n)]
    for f in frames:
        f[..., 3] = 255
    layers = layers_of(rng, n, L, h, w)
    got, t = ctx.sequence_bilateral(frames, 8, SS, SC, layers=layers, out_dtype=np.uint8)
    assert _direct(ctx)
    assert_same(got, want_layers(ctx, frames, layers, 8, np.uint8))
