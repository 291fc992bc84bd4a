"""GPU suite: mid_sequence_atrous_joint -- an animation through the frame pipeline with the a-trous filter (section a4g) as its
compute stage.  Every comparison is on raw bits against the resident call (ctx.atrous_joint of frame t with frame t's layers),
which test_gpu_atrous_joint.py holds against the float64 checker; refusals leave host_out and timings_ms untouched; the cached
levels come back after mid_ctx_release_cached."""
import ctypes

import numpy as np
import pytest

import guide_format_inputs as gi
import image_denoising_filter_amd as mid
from test_gpu_kernel_bits import guide

pytestmark = pytest.mark.gpu

DT = (np.float32, np.uint8, np.float16)
SHAPE, N = (45, 70), 7                                   # ragged tiles; more frames than the 4-slot ring, both kernel streams busy
SIG = [1.0, 2.0, 0.5]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def assert_same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (i, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), f"output {i} differs"


def inputs(fdt, gdt, L=3):
    frames = gi.hdr_frames(SHAPE, N, seed=21)
    if fdt == np.uint8:
        frames = [np.clip(f * 60, 0, 255).astype(np.uint8) for f in frames]
    else:
        frames = [f.astype(fdt) for f in frames]
    if gdt == np.uint8:
        layers = [[guide(SHAPE, f, l) for l in range(L)] for f in range(N)]
    else:
        layers = [ls[:L] for ls in gi.render_layers(SHAPE, N, gdt)]
    return frames, layers


@pytest.mark.parametrize("gdt", DT, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("fdt", DT, ids=lambda d: np.dtype(d).name)
def test_the_sequence_call_gives_the_bits_of_the_resident_call(ctx, fdt, gdt):
    frames, layers = inputs(fdt, gdt)
    i = 0
    for passes, cs in ((1, 0.0), (2, 1.0), (5, 4.0)):    # no level, one level, both levels between the passes
        for odt in DT:
            want = [ctx.atrous_joint(f, ls, SIG, passes=passes, color_sigma=cs, out_dtype=odt) for f, ls in zip(frames, layers)]
            for pinned, pinned_out, overlap in ((True, True, True), (False, False, True), (True, False, False), (False, True, False)):
                if (i + pinned + 2 * overlap) % 2 and odt != np.float32:
                    continue                             # (every output format meets every memory kind over the three pass counts)
                got, t = ctx.sequence_atrous_joint(frames, layers, SIG, passes=passes, color_sigma=cs, overlap=overlap, pinned=pinned,
                                                   pinned_out=pinned_out, out_dtype=odt)
                assert_same(got, want)
                assert t[0] > 0 and t[1] > 0
            i += 1


def test_a_block_of_the_sequence_and_a_continued_filter(ctx):
    frames, layers = inputs(np.float32, np.float32)
    want = [ctx.atrous_joint(f, ls, SIG, passes=3, first_pass=2) for f, ls in zip(frames, layers)]
    got, _ = ctx.sequence_atrous_joint(frames, layers, SIG, passes=3, first_pass=2, first=2, count=4)
    assert_same(got, want[2:6])
    got, _ = ctx.sequence_atrous_joint(frames[:1], layers[:1], SIG, passes=8)
    assert_same(got, [ctx.atrous_joint(frames[0], layers[0], SIG, passes=8)])


def test_sixteen_layers_and_release_cached(ctx):
    frames, _ = inputs(np.float32, np.float32)
    layers = [[guide(SHAPE, f, l) for l in range(16)] for f in range(N)]
    sig = [0.5 + 0.1 * l for l in range(16)]
    want = [ctx.atrous_joint(f, ls, sig, passes=4) for f, ls in zip(frames, layers)]
    got, _ = ctx.sequence_atrous_joint(frames, layers, sig, passes=4)
    assert_same(got, want)
    ctx.release_cached()
    got, _ = ctx.sequence_atrous_joint(frames, layers, sig, passes=4, out_dtype=np.uint8)
    assert_same(got, [ctx.pack_u8(x) for x in want])
    ctx.release_cached()
    got, _ = ctx.sequence_atrous_joint(frames[:2], layers[:2], sig, passes=1)          # a call that needs no level
    assert_same(got, [ctx.atrous_joint(f, ls, sig, passes=1) for f, ls in zip(frames[:2], layers[:2])])


def test_refusals_leave_the_outputs_and_the_timings_untouched(ctx):
    h, w = SHAPE
    frames, layers = inputs(np.float32, np.float32, 2)
    frames, layers = frames[:3], layers[:3]
    flat = [l for ls in layers for l in ls]
    outs = [np.full((h, w, 4), 7.0, np.float32) for _ in range(3)]
    F32 = mid.FMT_RGBA32F
    base = dict(w=w, h=h, first_pass=0, n_passes=3, cs=0.0, fmt=mid.api.fmt_with_guide(F32, F32), sig=[0.5, 0.5],
                frames=[f.ctypes.data for f in frames], n=3, layers=[l.ctypes.data for l in flat], nl=2, first=0, count=3,
                outs=[o.ctypes.data for o in outs], ofmt=F32, null_p=False, null_frames=False, null_layers=False, null_outs=False)
    t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)

    def call(**kw):
        a = dict(base, **kw)
        p = mid.AtrousParams(a["w"], a["h"], a["first_pass"], a["n_passes"], a["cs"], a["fmt"])
        sig = None if a["sig"] is None else (ctypes.c_float * 16)(*a["sig"])
        fr = None if a["null_frames"] else (ctypes.c_void_p * 8)(*a["frames"])
        ly = None if a["null_layers"] else (ctypes.c_void_p * 64)(*a["layers"])
        ou = None if a["null_outs"] else (ctypes.c_void_p * 8)(*a["outs"])
        return mid.lib.mid_sequence_atrous_joint(ctx.handle, None if a["null_p"] else ctypes.byref(p), sig, fr, a["n"], ly, a["nl"], a["first"],
                                                 a["count"], ou, a["ofmt"], 1, t)

    nan = float("nan")
    refused = {
        "NULL params": dict(null_p=True), "NULL sigmas": dict(sig=None), "NULL frame table": dict(null_frames=True),
        "NULL layer table": dict(null_layers=True), "NULL output table": dict(null_outs=True),
        "NULL frame": dict(frames=[base["frames"][0], None, base["frames"][2]]), "NULL layer": dict(layers=base["layers"][:3] + [None] + base["layers"][4:]),
        "NULL output": dict(outs=[base["outs"][0], None, base["outs"][2]]),
        "no layers": dict(nl=0), "17 layers": dict(nl=17), "sigma 0": dict(sig=[0.5, 0.0]), "sigma NaN": dict(sig=[nan, 0.5]),
        "colorSigma < 0": dict(cs=-0.5), "colorSigma NaN": dict(cs=nan), "no passes": dict(n_passes=0), "nine passes": dict(n_passes=9),
        "first_pass < 0": dict(first_pass=-1), "passes beyond 8": dict(first_pass=7, n_passes=2),
        "unknown frame format": dict(fmt=3), "unknown guide code": dict(fmt=F32 | (9 << 8)), "unknown output format": dict(ofmt=4),
        "no frames": dict(n=0, count=0), "first < 0": dict(first=-1), "count 0": dict(count=0), "range beyond the frames": dict(first=2, count=2),
        "output is a frame": dict(outs=[base["frames"][1]] + base["outs"][1:]), "output is a layer": dict(outs=base["outs"][:2] + [base["layers"][0]]),
        "output twice": dict(outs=[base["outs"][0], base["outs"][0], base["outs"][2]]),
        "width 0": dict(w=0), "height < 0": dict(h=-1),
    }
    for name, kw in refused.items():
        assert call(**kw) == 1, name
        assert mid.lib.mid_last_error(), name
        assert list(t) == [-1.0, -1.0, -1.0], name
    # inside a recording: the resident call is recorded (it only enqueues on the one stream), the sequence call is refused
    d_in, d_l, d_out = ctx.upload(frames[0]), [ctx.upload(l) for l in layers[0]], ctx.alloc(h * w * 16)
    p1 = mid.AtrousParams(w, h, 0, 1, 0.0, base["fmt"])
    with ctx.record(None) as rec:
        assert mid.lib.mid_atrous_joint(ctx.handle, ctypes.byref(p1), (ctypes.c_float * 2)(0.5, 0.5), d_in.ptr,
                                        (ctypes.c_void_p * 2)(*[d.ptr for d in d_l]), 2, d_out.ptr, F32, None, None) == 0
        assert call() == 1 and b"mid_sequence_atrous_joint" in mid.lib.mid_last_error() and b"recording" in mid.lib.mid_last_error()
    rec.submit(None)
    ctx.sync(None)
    rec.close()
    assert_same([ctx.download(d_out, (h, w, 4), np.float32)], [ctx.atrous_joint(frames[0], layers[0], [0.5, 0.5], passes=1)])
    assert all((o == 7.0).all() for o in outs) and list(t) == [-1.0, -1.0, -1.0]
    assert call() == 0 and t[0] > 0
    assert_same(outs, [ctx.atrous_joint(f, ls, [0.5, 0.5], passes=3) for f, ls in zip(frames, layers)])
