"""GPU suite: the recursive a-trous sequence with the firefly clamp in front (mid_sequence_atrous_recursive_firefly, section a4l).

The cases of tests/test_gpu_sequence_atrous_recursive_albedo.py -- eight frames of 131 x 67, two passes, both feedback values, with
and without motion, WITH AND WITHOUT ALBEDO, overlap 0 / 1, sub-ranges with warm-up, pageable and page-locked host memory, u8 /
f16 / f32 outputs -- on frames that hold fireflies of 4096 x, NaN and +-Inf channels.  Every output must equal, BIT FOR BIT, the
chain of public calls [demodulate ->] firefly_clamp -> atrous_moments -> temporal_accumulate -> atrous_variance [-> modulate].
firefly_rank=0 gives the bits of the existing call.  Refusals leave host_out untouched.  And the point of it all, twice: a firefly
and a NaN texel leave no trace in a run with the stage, and stay for good in a run without it.
"""
import ctypes

import numpy as np
import pytest

import image_denoising_filter_amd as mid
import temporal_accumulate_inputs as tai
from firefly_inputs import plant
from test_gpu_atrous_bounds import same
from test_gpu_sequence_atrous_recursive_albedo import ALBEDO, FLOOR, LAYERS, MOTION

pytestmark = pytest.mark.gpu

SHAPE, N, L, PASSES = (67, 131), 8, 3, 2
SG = tai.sigmas_of(L)
ACC = dict(alpha=0.2, alpha_moments=0.25, history_max=6, history_full=3)
VAR = dict(sigma_lum=4.0, epsilon=1e-3)
FF = dict(radius=2, rank=2, gain=1.5, floor=0.125)
FFKW = {"firefly_" + k: v for k, v in FF.items()}


def frames_of(dt=np.float32):
    """tai's frames; the float ones with fireflies, NaN and +-Inf channels on the corners, the tile seams and inside (odd frames)."""
    fr = [tai.frame_of(SHAPE, t, dt) for t in range(N)]
    if np.dtype(dt) != np.uint8:
        fr = [plant(f, (0, 15, 16, 40, 66), (0, 63, 64, 100, 130)) if t % 2 else f for t, f in enumerate(fr)]
    return fr


CHAINS = {}


def chain(ctx, fdt, with_motion, feedback, odt, albedo, start=0):
    """The outputs of frames start .. N-1 by public calls, the history starting at frame `start`."""
    key = (np.dtype(fdt).name, with_motion, feedback, np.dtype(odt).name, albedo, start)
    if key not in CHAINS:
        fr, hist, outs = frames_of(fdt), None, []
        for t in range(start, N):
            il = ctx.demodulate(fr[t], ALBEDO[t], FLOOR) if albedo else fr[t]
            cl = ctx.firefly_clamp(il, **FF)
            assert cl.dtype == np.float32 and np.isfinite(cl).all()
            vs = ctx.atrous_moments([cl], [LAYERS[t]], SG, k=0, t=0)
            col, st, var = ctx.temporal_accumulate(cl, LAYERS[t], LAYERS[t - 1] if hist is not None else LAYERS[t], SG, hist=hist,
                                                   motion=MOTION[t] if with_motion else None, var_spatial=vs, **ACC)
            last = dict(out_dtype=np.float32 if albedo else odt)
            if feedback == 0:
                fin = ctx.atrous_variance(col, var, LAYERS[t], SG, passes=PASSES, **last, **VAR)
                hist = (col, st)
            else:
                lvl, v1 = ctx.atrous_variance(col, var, LAYERS[t], SG, passes=1, return_variance=True, **VAR)
                fin = ctx.atrous_variance(lvl, v1, LAYERS[t], SG, passes=PASSES - 1, first_pass=1, **last, **VAR)
                hist = (lvl, st)
            outs.append(ctx.modulate(fin, ALBEDO[t], FLOOR, out_dtype=odt) if albedo else fin)
        CHAINS[key] = outs
    return CHAINS[key]


def run(ctx, fdt, with_motion, feedback, odt, albedo, frames=slice(None), ff=FFKW, **kw):
    fr = frames_of(fdt)[frames]
    outs, _ = ctx.sequence_atrous_recursive(fr, LAYERS[frames], SG, motion=MOTION[frames] if with_motion else None, feedback=feedback, passes=PASSES,
                                            out_dtype=odt, albedo=ALBEDO[frames] if albedo else None, albedo_floor=FLOOR, **ff, **ACC, **VAR, **kw)
    return outs


def test_the_frames_hold_what_the_docstring_says():
    fr = frames_of()
    assert all(np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any() and f[np.isfinite(f)].max() > 1000 for f in fr[1::2])
    assert all(np.isfinite(f).all() for f in fr[0::2])


@pytest.mark.parametrize("albedo", (False, True), ids=("colour", "illumination"))
@pytest.mark.parametrize("feedback", (0, 1))
@pytest.mark.parametrize("with_motion", (False, True), ids=("still", "motion"))
def test_every_output_is_the_chain_of_public_calls(ctx, with_motion, feedback, albedo):
    want = chain(ctx, np.float32, with_motion, feedback, np.float32, albedo)
    assert all(np.isfinite(w).all() for w in want)
    for overlap in (1, 0):
        got = run(ctx, np.float32, with_motion, feedback, np.float32, albedo, overlap=bool(overlap))
        assert len(got) == N and all(same(g, w) for g, w in zip(got, want)), (with_motion, feedback, albedo, overlap)
    assert not same(want[-1], chain(ctx, np.float32, with_motion, feedback, np.float32, not albedo)[-1])           # (the albedo matters)
    assert not same(want[-1], run(ctx, np.float32, with_motion, feedback, np.float32, albedo, ff={})[-1])           # (and the stage)
    other = dict(FFKW, firefly_rank=1)
    assert not same(want[-1], run(ctx, np.float32, with_motion, feedback, np.float32, albedo, ff=other)[-1])        # (and its rank)


@pytest.mark.parametrize("albedo", (False, True), ids=("colour", "illumination"))
@pytest.mark.parametrize("warmup", (0, 2, 8))
def test_a_sub_range_with_warm_up(ctx, warmup, albedo):
    first, count = 3, 2
    s = max(0, first - warmup)
    for feedback in (0, 1):
        got = run(ctx, np.float32, True, feedback, np.float32, albedo, first=first, count=count, warmup=warmup)
        want = chain(ctx, np.float32, True, feedback, np.float32, albedo, start=s)[first - s:first - s + count]
        assert len(got) == count and all(same(g, w) for g, w in zip(got, want)), (warmup, feedback)
        whole = chain(ctx, np.float32, True, feedback, np.float32, albedo)[first:first + count]
        assert all(same(g, w) for g, w in zip(got, whole)) == (s == 0), warmup


@pytest.mark.parametrize("albedo", (False, True), ids=("colour", "illumination"))
@pytest.mark.parametrize("odt", (np.uint8, np.float16, np.float32), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("pinned_out", (False, True), ids=("pageable", "pinned"))
def test_output_formats_and_host_memory_kinds(ctx, pinned_out, odt, albedo):
    fdt = np.uint8 if odt == np.uint8 else np.float16 if odt == np.float16 else np.float32
    want = chain(ctx, fdt, True, 1, odt, albedo)
    for pinned in (False, True):
        got = run(ctx, fdt, True, 1, odt, albedo, pinned=pinned, pinned_out=pinned_out, first=2, count=5, warmup=4)
        assert all(g.dtype == np.dtype(odt) and same(g, w) for g, w in zip(got, want[2:7])), (pinned, pinned_out)


def test_rank_0_is_the_existing_call(ctx):
    fr = [tai.frame_of(SHAPE, t, np.float32) for t in range(N)]
    kw = dict(motion=MOTION, feedback=1, passes=PASSES, **ACC, **VAR)
    for alb in (None, ALBEDO):
        plain, _ = ctx.sequence_atrous_recursive(fr, LAYERS, SG, albedo=alb, albedo_floor=FLOOR, **kw)
        off, _ = ctx.sequence_atrous_recursive(fr, LAYERS, SG, albedo=alb, albedo_floor=FLOOR, firefly_rank=0, **kw)
        on, _ = ctx.sequence_atrous_recursive(fr, LAYERS, SG, albedo=alb, albedo_floor=FLOOR, firefly_rank=1, **kw)
        assert all(same(a, b) for a, b in zip(plain, off))
        assert not same(plain[-1], on[-1])                                  # (noisy frames: the brightest pixel of every window is clamped)
    with pytest.raises(ValueError):
        ctx.sequence_atrous_recursive(fr, LAYERS, SG, firefly_gain=2.0, **kw)


# ---- the two demonstrations: a constant frame, one constant layer, sigma_lum 4, five passes, feedback 1 -------------------------------
C0 = np.float32([0.375, 0.5, 0.25, 1.0])
DEMO = dict(passes=5, sigma_lum=4.0, feedback=1)


def demo_run(ctx, frames, **kw):
    layers = [[np.full(SHAPE + (4,), 0.5, np.float32)] for _ in frames]
    return ctx.sequence_atrous_recursive(frames, layers, [0.1], **DEMO, **kw)[0]


def test_a_firefly_leaves_no_trace(ctx):
    """Frame 3 holds one texel of 4096 x c.  The clamp at rank 1 returns the constant frame bit for bit (s = 2^-12 exactly), so every
    output is the clean sequence's, bit for bit; without the stage the blob is still in the history at frame 7."""
    clean = [np.broadcast_to(C0, SHAPE + (4,)).copy() for _ in range(N)]
    dirty = [f.copy() for f in clean]
    dirty[3][30, 70, :3] *= np.float32(4096)
    want = demo_run(ctx, clean)
    assert all(same(a, b) for a, b in zip(demo_run(ctx, clean, firefly_rank=1), want)), "the stage leaves a clean sequence alone"
    assert all(same(a, b) for a, b in zip(demo_run(ctx, dirty, firefly_rank=1), want))
    without = demo_run(ctx, dirty)
    assert all(same(a, b) for a, b in zip(without[:3], want[:3]))
    d = np.abs(without[7].astype(np.float64) - want[7])
    print(f"without the stage, frame 7 is up to {d.max():.3e} from the clean sequence, at {(d > 1e-3).any(-1).sum()} pixels")
    assert d.max() > 1e-3


def test_a_nan_leaves_no_trace(ctx):
    """Frame 2 holds one NaN channel.  Without the stage every output from frame 2 on holds NaN (the behaviour as shipped); with it
    every output is finite and within 1e-5 max(1, |ref|) of the clean run: the repaired grey differs from c only by the rounding
    of l()."""
    grey = np.broadcast_to(np.float32([0.4, 0.4, 0.4, 1.0]), SHAPE + (4,))    # c grey: the repaired pixel is l(c) in R, G and B
    clean = [grey.copy() for _ in range(N)]
    dirty = [f.copy() for f in clean]
    dirty[2][30, 70, 1] = np.nan
    want = demo_run(ctx, clean)
    without = demo_run(ctx, dirty)
    assert all(np.isfinite(o).all() for o in without[:2]) and all(np.isnan(o).any() for o in without[2:])
    got = demo_run(ctx, dirty, firefly_rank=1)
    assert all(np.isfinite(o).all() for o in got)
    err = max(float(np.max(np.abs(g.astype(np.float64) - r) / np.maximum(1.0, np.abs(r)))) for g, r in zip(got, want))
    print(f"with the stage, the sequence with a NaN texel is within {err:.3e} of the clean run")
    assert err <= 1e-5


def test_refusals_leave_the_outputs_untouched(ctx):
    fr = frames_of()
    h, w = SHAPE
    flat = [l for ls in LAYERS for l in ls]
    outs = [np.full((h, w, 4), 7.0, np.float32) for _ in range(N)]
    hin, hl, hout = ([a.ctypes.data for a in arrs] for arrs in (fr, flat, outs))
    ap = mid.TemporalAccumParams(w, h, 0.2, 0.25, 6, 3, mid.FMT_RGBA32F)
    vp = mid.AtrousVarianceParams(w, h, 0, PASSES, 4.0, 1e-3, mid.FMT_RGBA32F)
    sg = (ctypes.c_float * L)(*SG)

    def call(fp):
        t = (ctypes.c_float * 3)()
        return mid.lib.mid_sequence_atrous_recursive_firefly(ctx.handle, ctypes.byref(ap), ctypes.byref(vp), sg, (ctypes.c_void_p * N)(*hin), N,
                                                             (ctypes.c_void_p * len(hl))(*hl), L, None, None, 0.0, ctypes.byref(fp), 1, 16, 0, N,
                                                             (ctypes.c_void_p * N)(*hout), mid.FMT_RGBA32F, 1, t)

    def refused(*words, **kw):
        args = dict(width=w, height=h, radius=1, rank=1, gain=1.0, floor=0.0, format=mid.FMT_RGBA32F)
        args.update(kw)
        rc = call(mid.FireflyParams(*[args[k] for k in ("width", "height", "radius", "rank", "gain", "floor", "format")]))
        msg = mid.lib.mid_last_error().decode()
        assert rc == 1 and all(x in msg for x in words) and "sequence_atrous_recursive_firefly" in msg, (rc, msg)
        assert all((o == 7.0).all() for o in outs), "an output was touched"

    refused(f"{w + 1}x{h}", f"{w}x{h}", width=w + 1)
    refused(f"{w}x{h - 1}", f"{w}x{h}", height=h - 1)
    refused("0x1", "format 0", format=mid.FMT_RGBA8)                       # the frames are RGBA32F: both values are named
    refused("guide bits", format=mid.FMT_RGBA32F | (3 << 8))
    refused("radius", radius=3)
    refused("rank", rank=0)
    refused("rank", rank=5)
    refused("gain", gain=0.0)
    refused("gain", gain=float("nan"))
    refused("floor", floor=-1.0)
    refused("floor", floor=float("inf"))
    # and the valid call still runs into these buffers
    assert call(mid.FireflyParams(w, h, FF["radius"], FF["rank"], FF["gain"], FF["floor"], mid.FMT_RGBA32F)) == 0, mid.lib.mid_last_error()
    want = chain(ctx, np.float32, False, 1, np.float32, False)
    assert all(same(o, c) for o, c in zip(outs, want))
