"""GPU suite: mid_sequence_atrous_joint_temporal -- an animation through the frame pipeline with the a-trous filter over
neighbouring frames (section a4h) as its compute stage.  Every comparison is on raw bits against the resident call
(ctx.atrous_joint_temporal), which test_gpu_atrous_temporal.py holds against the float64 checker; refusals leave host_out and
timings_ms untouched; a call inside a recording is refused."""
import ctypes

import numpy as np
import pytest

import guide_format_inputs as gi
import image_denoising_filter_amd as mid
from test_gpu_kernel_bits import guide

pytestmark = pytest.mark.gpu

DT = (np.float32, np.uint8, np.float16)
SHAPE, N = (21, 70), 6                                   # ragged tiles in both tile heights; more frames than a window of k = 2
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
        sets = [gi.render_layers(SHAPE, N, gdt, seed=12 + s) for s in range((L + 2) // 3)]
        layers = [[sets[l // 3][f][l % 3] for l in range(L)] for f in range(N)]
    return frames, layers


@pytest.mark.parametrize("gdt", DT, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("fdt", DT, ids=lambda d: np.dtype(d).name)
def test_the_sequence_call_gives_the_bits_of_the_resident_call(ctx, fdt, gdt):
    frames, layers = inputs(fdt, gdt)
    i = 0
    # no level, one level, both levels between the passes; the whole sequence and sub-ranges whose halo is clipped at neither,
    # one or both ends
    for passes, cs, k, first, count in ((1, 0.0, 1, 0, N), (2, 1.0, 2, 1, 4), (5, 4.0, 2, 3, 3)):
        for odt in DT:
            kw = dict(k=k, first=first, count=count, passes=passes, color_sigma=cs, out_dtype=odt)
            want = ctx.atrous_joint_temporal(frames, layers, SIG, **kw)
            for pinned, pinned_out, overlap in ((True, True, True), (False, False, True), (True, False, False), (False, True, False)):
                if (i + pinned + 2 * overlap) % 2 and odt != np.float32:
                    continue                             # (every output format meets every memory kind over the three cases)
                got, t = ctx.sequence_atrous_joint_temporal(frames, layers, SIG, overlap=overlap, pinned=pinned, pinned_out=pinned_out, **kw)
                assert_same(got, want)
                assert t[0] > 0 and t[1] > 0
            i += 1


@pytest.mark.parametrize("L", [4, 16])
def test_the_other_classes_and_k0(ctx, L):
    frames, layers = inputs(np.float32, np.uint8, L)
    sig = [0.5 + 0.1 * l for l in range(L)]
    for k, passes in ((2, 3), (0, 2)):
        want = ctx.atrous_joint_temporal(frames, layers, sig, k=k, passes=passes)
        got, _ = ctx.sequence_atrous_joint_temporal(frames, layers, sig, k=k, passes=passes)
        assert_same(got, want)
    assert_same(want, [ctx.atrous_joint(f, ls, sig, passes=2) for f, ls in zip(frames, layers)])


def test_refusals_leave_the_outputs_and_the_timings_untouched(ctx):
    h, w = SHAPE
    frames, layers = inputs(np.float32, np.float32, 2)
    frames, layers = frames[:3], layers[:3]
    flat = [l for ls in layers for l in ls]
    outs = [np.full((h, w, 4), 7.0, np.float32) for _ in range(3)]
    F32 = mid.FMT_RGBA32F
    base = dict(w=w, h=h, first_pass=0, n_passes=3, cs=0.0, fmt=mid.api.fmt_with_guide(F32, F32), sig=[0.5, 0.5],
                frames=[f.ctypes.data for f in frames], n=3, layers=[l.ctypes.data for l in flat], nl=2, k=1, first=0, count=3,
                outs=[o.ctypes.data for o in outs], ofmt=F32, null_p=False, null_frames=False, null_layers=False, null_outs=False)
    t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)

    def call(**kw):
        a = dict(base, **kw)
        p = mid.AtrousParams(a["w"], a["h"], a["first_pass"], a["n_passes"], a["cs"], a["fmt"])
        sig = None if a["sig"] is None else (ctypes.c_float * 17)(*a["sig"])
        fr = None if a["null_frames"] else (ctypes.c_void_p * 16)(*a["frames"])
        ly = None if a["null_layers"] else (ctypes.c_void_p * 256)(*a["layers"])
        ou = None if a["null_outs"] else (ctypes.c_void_p * 8)(*a["outs"])
        return mid.lib.mid_sequence_atrous_joint_temporal(ctx.handle, None if a["null_p"] else ctypes.byref(p), sig, fr, a["n"], ly, a["nl"],
                                                          a["k"], a["first"], a["count"], ou, a["ofmt"], 1, t)

    nan = float("nan")
    refused = {
        "NULL params": dict(null_p=True), "NULL sigmas": dict(sig=None), "NULL frame table": dict(null_frames=True),
        "NULL layer table": dict(null_layers=True), "NULL output table": dict(null_outs=True),
        "NULL frame": dict(frames=[base["frames"][0], None, base["frames"][2]]), "NULL layer": dict(layers=base["layers"][:3] + [None] + base["layers"][4:]),
        "NULL output": dict(outs=[base["outs"][0], None, base["outs"][2]]),
        "no layers": dict(nl=0), "17 layers": dict(nl=17), "sigma 0": dict(sig=[0.5, 0.0]), "sigma NaN": dict(sig=[nan, 0.5]),
        "colorSigma < 0": dict(cs=-0.5), "colorSigma NaN": dict(cs=nan), "no passes": dict(n_passes=0), "nine passes": dict(n_passes=9),
        "first_pass < 0": dict(first_pass=-1), "first_pass 1": dict(first_pass=1), "k < 0": dict(k=-1),
        "187 pointers": dict(n=11, k=5, nl=16, frames=[base["frames"][0]] * 11, layers=[base["layers"][0]] * 176, sig=[0.5] * 16, first=5, count=1),
        "unknown frame format": dict(fmt=3), "unknown guide code": dict(fmt=F32 | (9 << 8)), "unknown output format": dict(ofmt=4),
        "no frames": dict(n=0, count=0), "first < 0": dict(first=-1), "count 0": dict(count=0), "range beyond the frames": dict(first=2, count=2),
        "output is a frame": dict(outs=[base["frames"][1]] + base["outs"][1:]), "output is a layer": dict(outs=base["outs"][:2] + [base["layers"][0]]),
        "output is a halo frame": dict(first=0, count=1, outs=[base["frames"][1]]),
        "output twice": dict(outs=[base["outs"][0], base["outs"][0], base["outs"][2]]),
        "width 0": dict(w=0), "height < 0": dict(h=-1),
    }
    for name, kw in refused.items():
        assert call(**kw) == 1, name
        assert mid.lib.mid_last_error(), name
        assert list(t) == [-1.0, -1.0, -1.0], name
    # inside a recording: the resident call is recorded (it only enqueues on the one stream), the sequence call is refused
    d_fr = [ctx.upload(f) for f in frames]
    d_l = [ctx.upload(l) for l in flat]
    d_out = ctx.alloc(h * w * 16)
    p1 = mid.AtrousParams(w, h, 0, 1, 0.0, base["fmt"])
    with ctx.record(None) as rec:
        assert mid.lib.mid_atrous_joint_temporal(ctx.handle, ctypes.byref(p1), (ctypes.c_float * 2)(0.5, 0.5), (ctypes.c_void_p * 3)(*[d.ptr for d in d_fr]),
                                                 (ctypes.c_void_p * 6)(*[d.ptr for d in d_l]), 2, 3, 1, 1, 1, (ctypes.c_void_p * 1)(d_out.ptr), F32,
                                                 None, None) == 0
        assert call() == 1 and b"mid_sequence_atrous_joint_temporal" in mid.lib.mid_last_error() and b"recording" in mid.lib.mid_last_error()
    rec.submit(None)
    ctx.sync(None)
    rec.close()
    assert_same([ctx.download(d_out, (h, w, 4), np.float32)], ctx.atrous_joint_temporal(frames, layers, [0.5, 0.5], k=1, first=1, count=1, passes=1))
    assert all((o == 7.0).all() for o in outs) and list(t) == [-1.0, -1.0, -1.0]
    assert call() == 0 and t[0] > 0
    assert_same(outs, ctx.atrous_joint_temporal(frames, layers, [0.5, 0.5], k=1, passes=3))
