"""GPU suite: mid_sequence_guided -- an animation through the frame pipeline with the guided filter (section a4o) as its compute
stage.  Every comparison is on raw bits against the resident call (ctx.guided_filter of frame t with frame t's guide), which
test_gpu_guided.py holds against the float64 checker: with and without guides, first > 0, overlap 0 and 1, pageable and page-locked
frames, the three output formats; the cached workspace comes back after mid_ctx_release_cached; refusals leave host_out and
timings_ms untouched."""
import ctypes

import numpy as np
import pytest

import guided_inputs as gi
import image_denoising_filter_amd as mid

pytestmark = pytest.mark.gpu

DT = (np.float32, np.uint8, np.float16)
SHAPE, N = (45, 70), 7                                   # more frames than the 4-slot ring, both kernel streams busy
RADIUS = 3


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def assert_same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (i, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), f"output {i} differs"


def inputs(fdt, gdt):
    scenes = [gi.scene(SHAPE[0], SHAPE[1], RADIUS, seed=40 + t) for t in range(N)]
    frames = [gi.as_dtype(s[0], fdt) for s in scenes]
    guides = None if gdt is None else [gi.as_dtype(s[1], gdt) for s in scenes]
    return frames, guides


@pytest.mark.parametrize("gdt", DT + (None,), ids=lambda d: "self" if d is None else np.dtype(d).name)
@pytest.mark.parametrize("fdt", DT, ids=lambda d: np.dtype(d).name)
def test_the_sequence_call_gives_the_bits_of_the_resident_call(ctx, fdt, gdt):
    frames, guides = inputs(fdt, gdt)
    for i, odt in enumerate(DT):
        want = [ctx.guided_filter(f, None if guides is None else guides[t], RADIUS, gi.EPS, out_dtype=odt) for t, f in enumerate(frames)]
        for pinned, overlap in ((True, True), (False, True), (True, False), (False, False)):
            if (i + pinned + overlap) % 2 and odt != np.float32:
                continue                                 # (every output format meets every memory kind over the format pairs)
            got, t = ctx.sequence_guided(frames, guides, RADIUS, gi.EPS, overlap=overlap, pinned=pinned, out_dtype=odt)
            assert_same(got, want)
            assert t[0] > 0 and t[1] > 0


def test_a_block_of_the_sequence_and_release_cached(ctx):
    frames, guides = inputs(np.float32, np.uint8)
    want = [ctx.guided_filter(f, g, 16, 1e-2) for f, g in zip(frames, guides)]
    got, _ = ctx.sequence_guided(frames, guides, 16, 1e-2, first=2, count=4)
    assert_same(got, want[2:6])
    ctx.release_cached()
    got, _ = ctx.sequence_guided(frames, guides, 16, 1e-2, first=N - 1, out_dtype=np.uint8)
    assert_same(got, [ctx.pack_u8(want[-1])])
    got, _ = ctx.sequence_guided(frames[:1], None, 1, 1e-2)
    assert_same(got, [ctx.guided_filter(frames[0], None, 1, 1e-2)])


def test_refusals_leave_the_outputs_and_the_timings_untouched(ctx):
    h, w = SHAPE
    frames, guides = inputs(np.float32, np.float32)
    frames, guides = frames[:3], guides[:3]
    outs = [np.full((h, w, 4), 7.0, np.float32) for _ in range(3)]
    F32 = mid.FMT_RGBA32F
    base = dict(w=w, h=h, radius=RADIUS, eps=1e-2, fmt=mid.api.fmt_with_guide(F32, F32), frames=[f.ctypes.data for f in frames], n=3,
                guides=[g.ctypes.data for g in guides], first=0, count=3, outs=[o.ctypes.data for o in outs], ofmt=F32, null_p=False,
                null_frames=False, null_outs=False)
    t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)

    def call(**kw):
        a = dict(base, **kw)
        p = mid.GuidedParams(a["w"], a["h"], a["radius"], a["eps"], a["fmt"])
        fr = None if a["null_frames"] else (ctypes.c_void_p * 8)(*a["frames"])
        gd = None if a["guides"] is None else (ctypes.c_void_p * 8)(*a["guides"])
        ou = None if a["null_outs"] else (ctypes.c_void_p * 8)(*a["outs"])
        return mid.lib.mid_sequence_guided(ctx.handle, None if a["null_p"] else ctypes.byref(p), fr, a["n"], gd, a["first"], a["count"], ou,
                                           a["ofmt"], 1, t)

    nan = float("nan")
    refused = {
        "NULL params": dict(null_p=True), "NULL frame table": dict(null_frames=True), "NULL output table": dict(null_outs=True),
        "NULL frame": dict(frames=[base["frames"][0], None, base["frames"][2]]), "NULL guide": dict(guides=[base["guides"][0], None, base["guides"][2]]),
        "NULL output": dict(outs=[base["outs"][0], None, base["outs"][2]]),
        "radius 0": dict(radius=0), "radius 17": dict(radius=17), "eps 0": dict(eps=0.0), "eps NaN": dict(eps=nan), "eps Inf": dict(eps=float("inf")),
        "unknown frame format": dict(fmt=3), "unknown guide code": dict(fmt=F32 | (9 << 8)), "bits above 15": dict(fmt=base["fmt"] | (1 << 16)),
        "unknown output format": dict(ofmt=4),
        "no frames": dict(n=0, count=0), "first < 0": dict(first=-1), "count 0": dict(count=0), "range beyond the frames": dict(first=2, count=2),
        "output is a frame": dict(outs=[base["frames"][1]] + base["outs"][1:]), "output is a guide": dict(outs=base["outs"][:2] + [base["guides"][0]]),
        "output twice": dict(outs=[base["outs"][0], base["outs"][0], base["outs"][2]]),
        "width 0": dict(w=0), "height < 0": dict(h=-1),
    }
    for name, kw in refused.items():
        assert call(**kw) == 1, name
        assert mid.lib.mid_last_error(), name
        assert list(t) == [-1.0, -1.0, -1.0], name
    # inside a recording: the resident call is recorded (it only enqueues on the one stream), the sequence call is refused
    p1 = mid.GuidedParams(w, h, RADIUS, 1e-2, base["fmt"])
    d_in, d_g, d_work, d_out = ctx.upload(frames[0]), ctx.upload(guides[0]), ctx.alloc(52 * h * w), ctx.alloc(h * w * 16)
    with ctx.record(None) as rec:
        assert mid.lib.mid_guided_filter(ctx.handle, ctypes.byref(p1), d_in.ptr, d_g.ptr, d_work.ptr, d_out.ptr, F32, None) == 0
        assert call() == 1 and b"mid_sequence_guided" in mid.lib.mid_last_error() and b"recording" in mid.lib.mid_last_error()
    rec.submit(None)
    ctx.sync(None)
    rec.close()
    assert_same([ctx.download(d_out, (h, w, 4), np.float32)], [ctx.guided_filter(frames[0], guides[0], RADIUS, 1e-2)])
    assert all((o == 7.0).all() for o in outs) and list(t) == [-1.0, -1.0, -1.0]
    assert call() == 0 and t[0] > 0
    assert_same(outs, [ctx.guided_filter(f, g, RADIUS, 1e-2) for f, g in zip(frames, guides)])
    assert call(guides=None) == 0                        # no guide table: every frame guides itself
    assert_same(outs, [ctx.guided_filter(f, None, RADIUS, 1e-2) for f in frames])
