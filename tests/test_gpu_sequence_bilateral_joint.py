"""GPU suite: mid_sequence_bilateral_joint, the frame pipeline with the joint bilateral as its compute stage -- host frames and host
layers in, host frames out, every output with the BITS of the kernel-level call (mid_bilateral_joint) on the same inputs.

(20, 70) frames (a ragged 2 x 2 tile grid), five of them; k = 0 and 2; first / count sub-ranges; page-locked and pageable host
memory (pageable outputs between guard bytes); outputs float32 / uint8 / float16; RGBA8 and float32 layers; overlap 0 and 1; the
timeline export; the refusal inside a recording; the Python wrappers against the ctypes calls.
"""
import ctypes

import numpy as np
import pytest

import guide_format_inputs as gi
import image_denoising_filter_amd as mid
from test_gpu_kernel_bits import guide

pytestmark = pytest.mark.gpu

SHAPE, N, R = (20, 70), 5, 8
GUARD, GUARD_BYTE = 64, 0xA5
SIGMAS = {np.uint8: [0.2, 0.1, 0.3], np.float32: [1.0, 2.0, 0.5]}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def assert_same(got, want, what=""):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, i)
        assert np.array_equal(bits(g), bits(w)), f"{what}: output {i} differs"


def inputs(ldt):
    frames = gi.hdr_frames(SHAPE, N, seed=81, translucent=True)
    if ldt == np.uint8:
        layers = [[guide(SHAPE, f, l) for l in range(3)] for f in range(N)]
    else:
        layers = gi.render_layers(SHAPE, N, np.float32, seed=82)
    return frames, layers


def run_raw(ctx, frames, layers, sigmas, k, first, count, out_dt, pinned, overlap):
    """mid_sequence_bilateral_joint through ctypes on host buffers of this test's own, every output followed by GUARD bytes."""
    h, w = SHAPE
    flat = [l for ls in layers for l in ls]
    nbytes = h * w * 4 * np.dtype(out_dt).itemsize
    fmt = mid.api._guide_fmt(mid.api._fmt_of(frames[0]), flat, "test")
    out_fmt = {np.uint8: mid.FMT_RGBA8, np.float16: mid.FMT_RGBA16F, np.float32: mid.FMT_RGBA32F}[out_dt]
    hin = hlay = hout = None
    try:
        if pinned:
            hin, hlay, hout = mid.PinnedFrames(ctx, frames), mid.PinnedFrames(ctx, flat), mid.PinnedFrames(ctx, count, nbytes + GUARD)
            for p in hout.ptrs:
                ctypes.memset(p, GUARD_BYTE, nbytes + GUARD)
            pin, play, pout = hin.ptrs, hlay.ptrs, hout.ptrs
        else:
            bufs = [np.full(nbytes + GUARD, GUARD_BYTE, np.uint8) for _ in range(count)]
            pin, play, pout = [f.ctypes.data for f in frames], [l.ctypes.data for l in flat], [b.ctypes.data for b in bufs]
        prm = mid.BilateralParams(w, h, gi.SIGMA_S, 0.7, R, mid.LAYOUT_TEXTURE, fmt)
        t = (ctypes.c_float * 3)()
        sg = None if sigmas is None else (ctypes.c_float * len(sigmas))(*sigmas)
        rc = mid.lib.mid_sequence_bilateral_joint(ctx.handle, ctypes.byref(prm), sg, (ctypes.c_void_p * N)(*pin), N,
                                                  (ctypes.c_void_p * len(play))(*play), len(layers[0]), k, first, count,
                                                  (ctypes.c_void_p * count)(*pout[:count]), out_fmt, overlap, t)
        assert rc == 0, mid.lib.mid_last_error()
        outs = []
        for i in range(count):
            raw = np.ctypeslib.as_array((ctypes.c_uint8 * (nbytes + GUARD)).from_address(pout[i])).copy()
            assert (raw[nbytes:] == GUARD_BYTE).all(), f"the guard bytes behind output {i} were written"
            outs.append(raw[:nbytes].view(out_dt).reshape(h, w, 4))
        return outs
    finally:
        for b in (hin, hlay, hout):
            if b is not None:
                b.free()


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("ldt", [np.uint8, np.float32], ids=["u8-layers", "f32-layers"])
@pytest.mark.parametrize("k", [0, 2])
def test_pipeline_gives_the_kernel_level_bits(ctx, k, ldt, pinned):
    frames, layers = inputs(ldt)
    sig = SIGMAS[ldt]
    for j, out_dt in enumerate((np.float32, np.uint8, np.float16)):
        want = ctx.bilateral_joint(frames, layers, sig, k, radius=R, sigma_s=gi.SIGMA_S, out_dtype=out_dt)
        overlap = (j + k // 2) % 2
        assert_same(run_raw(ctx, frames, layers, sig, k, 0, N, out_dt, pinned, overlap), want, f"whole sequence, overlap {overlap}")
        assert_same(run_raw(ctx, frames, layers, sig, k, 1, 3, out_dt, pinned, 1 - overlap), want[1:4], "first=1 count=3")
        _, outs = ctx.pipe_last_timeline()
        assert [o[0] for o in outs] == [1, 2, 3]                                   # `count` outputs, from `first`
    assert_same(run_raw(ctx, frames, layers, sig, k, N - 1, 1, np.float32, pinned, 1),
                ctx.bilateral_joint(frames, layers, sig, k, N - 1, 1, radius=R, sigma_s=gi.SIGMA_S), "last frame alone")
    # layer_sigma NULL: colorSigma (0.7 here) in every layer
    assert_same(run_raw(ctx, frames, layers, None, k, 0, 2, np.float32, pinned, 1),
                ctx.bilateral_joint(frames, layers, None, k, 0, 2, radius=R, sigma_s=gi.SIGMA_S, sigma_c=0.7), "NULL sigmas")


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
def test_python_wrappers_agree_with_the_ctypes_calls(ctx, pinned):
    frames, layers = inputs(np.float32)
    sig = SIGMAS[np.float32]
    for k, out_dt in ((0, np.float32), (2, np.uint8), (1, np.float16)):
        got, times = ctx.sequence_bilateral_joint(frames, layers, sig, k, radius=R, sigma_s=gi.SIGMA_S, sigma_c=0.7, pinned=pinned,
                                                  pinned_out=pinned, out_dtype=out_dt)
        assert len(times) == 3 and times[0] > 0
        assert_same(got, run_raw(ctx, frames, layers, sig, k, 0, N, out_dt, pinned, 1), f"k={k}")
        ups, outs = ctx.pipe_last_timeline()
        assert [u[0] for u in ups] == list(range(N)) and [o[0] for o in outs] == list(range(N))
    sub, _ = ctx.sequence_bilateral_joint(frames, layers, sig, 1, first=2, count=2, radius=R, sigma_s=gi.SIGMA_S, pinned=pinned, pinned_out=pinned)
    assert_same(sub, ctx.bilateral_joint(frames, layers, sig, 1, 2, 2, radius=R, sigma_s=gi.SIGMA_S), "first=2 count=2")
    ups, outs = ctx.pipe_last_timeline()
    assert [u[0] for u in ups] == [1, 2, 3, 4] and [o[0] for o in outs] == [2, 3]


def test_refusals_queue_nothing(ctx):
    h, w = SHAPE
    frames, layers = inputs(np.float32)
    flat = [l for ls in layers for l in ls]
    L = 3
    outs = [np.full((h, w, 4), 7.0, np.float32) for _ in range(N)]
    t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    lib = mid.lib
    fmt = mid.api.fmt_with_guide(mid.FMT_RGBA32F, mid.FMT_RGBA32F)

    def raw(sigmas=(1.0, 2.0, 0.5), n_layers=L, table=True, k=1, first=0, count=N, layout=mid.LAYOUT_TEXTURE, out=None, out_fmt=mid.FMT_RGBA32F):
        p = mid.BilateralParams(w, h, 2.0, 0.2, 4, layout, fmt)
        sg = None if sigmas is None else (ctypes.c_float * len(sigmas))(*sigmas)
        out = [o.ctypes.data for o in outs] if out is None else out
        lt = (ctypes.c_void_p * max(n_layers * N, 1))(*[flat[i % len(flat)].ctypes.data for i in range(n_layers * N)]) if table else None
        return lib.mid_sequence_bilateral_joint(ctx.handle, ctypes.byref(p), sg, (ctypes.c_void_p * N)(*[f.ctypes.data for f in frames]), N,
                                                lt, n_layers, k, first, count, (ctypes.c_void_p * len(out))(*out), out_fmt, 1, t)

    ctx.sequence_bilateral_joint(frames, layers, [1.0, 2.0, 0.5], 1, radius=4)
    before = ctx.pipe_last_timeline()
    cases = {
        "n_layers 0": lambda: raw(n_layers=0, sigmas=None),
        "n_layers 17": lambda: raw(n_layers=17, sigmas=[0.5] * 17),
        "NULL layer table": lambda: raw(table=False),
        "sigma 0": lambda: raw(sigmas=(1.0, 0.0, 0.5)),
        "sigma negative": lambda: raw(sigmas=(1.0, 2.0, -0.5)),
        "sigma NaN": lambda: raw(sigmas=(float("nan"), 2.0, 0.5)),
        "linear layout": lambda: raw(layout=mid.LAYOUT_LINEAR),
        "k beyond the ring": lambda: raw(k=60),
        "unknown output format": lambda: raw(out_fmt=9),
        "k negative": lambda: raw(k=-1),
        "first negative": lambda: raw(first=-1),
        "count 0": lambda: raw(count=0),
        "first + count > n": lambda: raw(first=3, count=3),
        "an output is a frame": lambda: raw(out=[frames[1].ctypes.data] + [o.ctypes.data for o in outs[1:]]),
        "an output is a layer": lambda: raw(out=[flat[4].ctypes.data] + [o.ctypes.data for o in outs[1:]]),
        "an output twice": lambda: raw(out=[outs[0].ctypes.data] * N),
    }
    for name, call in cases.items():
        assert call() == 1, name
        assert lib.mid_last_error(), name
    d_in, d_out = ctx.upload(frames[0]), ctx.alloc(h * w * 16)
    with ctx.record() as rec:                                       # a recording with one launch in it, then the refused call
        ctx.bilateral_dev(d_in.ptr, d_out.ptr, w, h, 4, 2.0, 0.2, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)
        rc = raw()
    assert rec.info()[0] == 1
    rec.close()
    assert rc == 1 and b"recording" in lib.mid_last_error()
    assert all((o == 7.0).all() for o in outs) and list(t) == [-1.0, -1.0, -1.0]
    assert ctx.pipe_last_timeline() == before                       # no refused call queued anything
    assert raw() == 0, lib.mid_last_error()
    assert_same(outs, ctx.bilateral_joint(frames, layers, [1.0, 2.0, 0.5], 1, radius=4, sigma_s=2.0), "after the refusals")
