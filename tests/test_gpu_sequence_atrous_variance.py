"""GPU suite: mid_sequence_atrous_variance -- an animation through the frame pipeline with the variance-guided a-trous filter
(section a4i) as its compute stage.  Every comparison is on raw bits against the resident calls (ctx.atrous_moments over the
window, then ctx.atrous_variance on frame t), which test_gpu_atrous_moments.py and test_gpu_atrous_variance.py hold against the
float64 checker; refusals leave host_out and timings_ms untouched; a call inside a recording is refused."""
import ctypes

import numpy as np
import pytest

import atrous_variance_inputs as avi
import image_denoising_filter_amd as mid

pytestmark = pytest.mark.gpu

DT = (np.float32, np.uint8, np.float16)
SHAPE, N = (40, 70), 6                                   # 70 x 40: a ragged tile column, a ragged comb chunk; more frames than a window of k = 2


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def assert_same(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (i, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), f"output {i} differs"


def inputs(fdt, gdt, L=2):
    return [avi.frame_of(SHAPE, f, fdt) for f in range(N)], [avi.layers_of(SHAPE, L, gdt, f) for f in range(N)], avi.sigmas_of(L)


def resident(ctx, frames, layers, sig, k, first, count, **kw):
    return [ctx.atrous_variance(frames[t], ctx.atrous_moments(frames, layers, sig, k=k, t=t), layers[t], sig, **kw) for t in range(first, first + count)]


@pytest.mark.parametrize("fdt,gdt", [(np.float32, np.float32), (np.uint8, np.float16), (np.float16, np.uint8)],
                         ids=lambda d: np.dtype(d).name)
def test_the_sequence_call_gives_the_bits_of_the_resident_calls(ctx, fdt, gdt):
    frames, layers, sig = inputs(fdt, gdt)
    i = 0
    # no level, one set, both sets of levels between the passes; the whole sequence and the sub-ranges whose halo is clipped at
    # the start, at neither end, and at the end
    for passes, k, ranges in ((1, 1, ((0, N),)), (2, 2, ((0, 1), (2, 3), (5, 1))), (5, 2, ((0, N), (2, 3)))):
        for first, count in ranges:
            odt = DT[i % 3]
            kw = dict(passes=passes, sigma_lum=4.0, epsilon=1e-3, out_dtype=odt)
            want = resident(ctx, frames, layers, sig, k, first, count, **kw)
            for pinned, pinned_out, overlap in ((True, True, True), (False, False, True), (True, False, False), (False, True, False)):
                got, t = ctx.sequence_atrous_variance(frames, layers, sig, k=k, first=first, count=count, overlap=overlap, pinned=pinned,
                                                      pinned_out=pinned_out, **kw)
                assert_same(got, want)
                assert t[0] > 0 and t[1] > 0
            i += 1


@pytest.mark.parametrize("L", [4, 16])
def test_the_other_classes_and_k0(ctx, L):
    frames, layers, sig = inputs(np.float32, np.uint8, L)
    for k, passes, sl in ((2, 3, 1.0), (0, 2, 0.0)):
        want = resident(ctx, frames, layers, sig, k, 0, N, passes=passes, sigma_lum=sl)
        got, _ = ctx.sequence_atrous_variance(frames, layers, sig, k=k, passes=passes, sigma_lum=sl)
        assert_same(got, want)
    assert_same(want, [ctx.atrous_joint(f, ls, sig, passes=2) for f, ls in zip(frames, layers)])      # sigmaLum = 0: mid_atrous_joint's bits


def test_refusals_leave_the_outputs_and_the_timings_untouched(ctx):
    h, w = SHAPE
    frames, layers, _ = inputs(np.float32, np.float32, 2)
    frames, layers = frames[:3], layers[:3]
    flat = [l for ls in layers for l in ls]
    outs = [np.full((h, w, 4), 7.0, np.float32) for _ in range(3)]
    F32 = mid.FMT_RGBA32F
    base = dict(w=w, h=h, first_pass=0, n_passes=3, sl=4.0, eps=1e-3, fmt=mid.api.fmt_with_guide(F32, F32), sig=[0.5, 0.5],
                frames=[f.ctypes.data for f in frames], n=3, layers=[l.ctypes.data for l in flat], nl=2, k=1, first=0, count=3,
                outs=[o.ctypes.data for o in outs], ofmt=F32, null_p=False, null_frames=False, null_layers=False, null_outs=False)
    t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)

    def call(**kw):
        a = dict(base, **kw)
        p = mid.AtrousVarianceParams(a["w"], a["h"], a["first_pass"], a["n_passes"], a["sl"], a["eps"], a["fmt"])
        sig = None if a["sig"] is None else (ctypes.c_float * 17)(*a["sig"])
        fr = None if a["null_frames"] else (ctypes.c_void_p * 16)(*a["frames"])
        ly = None if a["null_layers"] else (ctypes.c_void_p * 256)(*a["layers"])
        ou = None if a["null_outs"] else (ctypes.c_void_p * 8)(*a["outs"])
        return mid.lib.mid_sequence_atrous_variance(ctx.handle, None if a["null_p"] else ctypes.byref(p), sig, fr, a["n"], ly, a["nl"],
                                                    a["k"], a["first"], a["count"], ou, a["ofmt"], 1, t)

    nan = float("nan")
    refused = {
        "NULL params": dict(null_p=True), "NULL sigmas": dict(sig=None), "NULL frame table": dict(null_frames=True),
        "NULL layer table": dict(null_layers=True), "NULL output table": dict(null_outs=True),
        "NULL frame": dict(frames=[base["frames"][0], None, base["frames"][2]]), "NULL layer": dict(layers=base["layers"][:3] + [None] + base["layers"][4:]),
        "NULL output": dict(outs=[base["outs"][0], None, base["outs"][2]]),
        "no layers": dict(nl=0), "17 layers": dict(nl=17), "sigma 0": dict(sig=[0.5, 0.0]), "sigma NaN": dict(sig=[nan, 0.5]),
        "sigmaLum < 0": dict(sl=-0.5), "sigmaLum NaN": dict(sl=nan), "epsilon 0": dict(eps=0.0), "epsilon NaN": dict(eps=nan),
        "no passes": dict(n_passes=0), "nine passes": dict(n_passes=9),
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
    # inside a recording: the resident calls are recorded (they only enqueue on the one stream), the sequence call is refused
    d_fr = [ctx.upload(f) for f in frames]
    d_l = [ctx.upload(l) for l in flat]
    d_var, d_out = ctx.alloc(h * w * 4), ctx.alloc(h * w * 16)
    mp = mid.AtrousMomentsParams(w, h, base["fmt"])
    p1 = mid.AtrousVarianceParams(w, h, 0, 1, 4.0, 1e-3, base["fmt"])
    sg = (ctypes.c_float * 2)(0.5, 0.5)
    with ctx.record(None) as rec:
        assert mid.lib.mid_atrous_moments(ctx.handle, ctypes.byref(mp), sg, (ctypes.c_void_p * 3)(*[d.ptr for d in d_fr]),
                                          (ctypes.c_void_p * 6)(*[d.ptr for d in d_l]), 2, 3, 1, 1, d_var.ptr, None) == 0
        assert mid.lib.mid_atrous_variance(ctx.handle, ctypes.byref(p1), sg, d_fr[1].ptr, d_var.ptr, (ctypes.c_void_p * 2)(d_l[2].ptr, d_l[3].ptr), 2,
                                           d_out.ptr, F32, None, None, None) == 0
        assert call() == 1 and b"mid_sequence_atrous_variance" in mid.lib.mid_last_error() and b"recording" in mid.lib.mid_last_error()
    rec.submit(None)
    ctx.sync(None)
    rec.close()
    assert_same([ctx.download(d_out, (h, w, 4), np.float32)], resident(ctx, frames, layers, [0.5, 0.5], 1, 1, 1, passes=1))
    assert all((o == 7.0).all() for o in outs) and list(t) == [-1.0, -1.0, -1.0]
    assert call() == 0 and t[0] > 0
    assert_same(outs, resident(ctx, frames, layers, [0.5, 0.5], 1, 0, 3, passes=3))
