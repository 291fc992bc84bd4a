"""GPU suite: the recursive a-trous sequence with the history clipped (mid_sequence_atrous_recursive_clip, section a4m).

The cases of tests/test_gpu_sequence_atrous_recursive_firefly.py -- eight frames of 131 x 67, two passes, both feedback values, with
and without motion, WITH AND WITHOUT ALBEDO, WITH AND WITHOUT THE FIREFLY CLAMP, overlap 0 / 1, sub-ranges with warm-up, pageable and
page-locked host memory, u8 / f16 / f32 outputs.  Every output must equal, BIT FOR BIT, the chain of public calls
[demodulate ->] [firefly_clamp ->] color_bounds -> atrous_moments -> temporal_accumulate(clip_lo, clip_hi) -> atrous_variance
[-> modulate], the box taken from the plane the accumulation reads.  clip_gamma=None gives the bits of the existing call.  Refusals
leave host_out untouched.  And the point of it all: when the lighting of a square changes and no layer does, the run with the clip
shows the new lighting on the frame of the change, and the run without it carries 0.8 of the step.
"""
import ctypes

import numpy as np
import pytest

import history_clip_inputs as hci
import image_denoising_filter_amd as mid
import temporal_accumulate_inputs as tai
from test_gpu_atrous_bounds import same
from test_gpu_sequence_atrous_recursive_albedo import ALBEDO, FLOOR, LAYERS, MOTION

pytestmark = pytest.mark.gpu

SHAPE, N, L, PASSES = (67, 131), 8, 3, 2
SG = tai.sigmas_of(L)
ACC = dict(alpha=0.2, alpha_moments=0.25, history_max=6, history_full=3)
VAR = dict(sigma_lum=4.0, epsilon=1e-3)
FF = dict(radius=2, rank=2, gain=1.5, floor=0.125)
FFKW = {"firefly_" + k: v for k, v in FF.items()}
CLIP = dict(radius=2, gamma=0.75)
CLIPKW = dict(clip_gamma=CLIP["gamma"], clip_radius=CLIP["radius"])
CHAINS = {}


def frames_of(dt=np.float32):
    return [tai.frame_of(SHAPE, t, dt) for t in range(N)]


def chain(ctx, fdt, with_motion, feedback, odt, albedo, firefly, start=0):
    """The outputs of frames start .. N-1 by public calls, the history starting at frame `start`."""
    key = (np.dtype(fdt).name, with_motion, feedback, np.dtype(odt).name, albedo, firefly, start)
    if key not in CHAINS:
        fr, hist, outs = frames_of(fdt), None, []
        for t in range(start, N):
            cur = ctx.demodulate(fr[t], ALBEDO[t], FLOOR) if albedo else fr[t]
            if firefly:
                cur = ctx.firefly_clamp(cur, **FF)
            if albedo or firefly:
                assert cur.dtype == np.float32                                       # the plane the accumulation reads is RGBA32F then
            lo, hi = ctx.color_bounds(cur, **CLIP)                                   # (frame `start` too: without history it clips nothing)
            vs = ctx.atrous_moments([cur], [LAYERS[t]], SG, k=0, t=0)
            col, st, var = ctx.temporal_accumulate(cur, LAYERS[t], LAYERS[t - 1] if hist is not None else LAYERS[t], SG, hist=hist,
                                                   motion=MOTION[t] if with_motion else None, var_spatial=vs, clip_lo=lo, clip_hi=hi, **ACC)
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


def run(ctx, fdt, with_motion, feedback, odt, albedo, firefly, frames=slice(None), clip=CLIPKW, **kw):
    fr = frames_of(fdt)[frames]
    outs, _ = ctx.sequence_atrous_recursive(fr, LAYERS[frames], SG, motion=MOTION[frames] if with_motion else None, feedback=feedback, passes=PASSES,
                                            out_dtype=odt, albedo=ALBEDO[frames] if albedo else None, albedo_floor=FLOOR, **(FFKW if firefly else {}),
                                            **clip, **ACC, **VAR, **kw)
    return outs


@pytest.mark.parametrize("firefly", (False, True), ids=("plain", "firefly"))
@pytest.mark.parametrize("albedo", (False, True), ids=("colour", "illumination"))
@pytest.mark.parametrize("feedback", (0, 1))
@pytest.mark.parametrize("with_motion", (False, True), ids=("still", "motion"))
def test_every_output_is_the_chain_of_public_calls(ctx, with_motion, feedback, albedo, firefly):
    want = chain(ctx, np.float32, with_motion, feedback, np.float32, albedo, firefly)
    for overlap in (1, 0):
        got = run(ctx, np.float32, with_motion, feedback, np.float32, albedo, firefly, overlap=bool(overlap))
        assert len(got) == N and all(same(g, w) for g, w in zip(got, want)), (with_motion, feedback, albedo, firefly, overlap)
    assert same(want[0], run(ctx, np.float32, with_motion, feedback, np.float32, albedo, firefly, clip={})[0])       # (frame 0 has nothing to clip)
    assert not same(want[-1], run(ctx, np.float32, with_motion, feedback, np.float32, albedo, firefly, clip={})[-1])  # (the clip matters)
    other = dict(CLIPKW, clip_radius=1)
    assert not same(want[-1], run(ctx, np.float32, with_motion, feedback, np.float32, albedo, firefly, clip=other)[-1])    # (and its radius)


@pytest.mark.parametrize("albedo", (False, True), ids=("colour", "illumination"))
@pytest.mark.parametrize("warmup", (0, 2, 8))
def test_a_sub_range_with_warm_up(ctx, warmup, albedo):
    first, count = 3, 2
    s = max(0, first - warmup)
    for feedback in (0, 1):
        got = run(ctx, np.float32, True, feedback, np.float32, albedo, True, first=first, count=count, warmup=warmup)
        want = chain(ctx, np.float32, True, feedback, np.float32, albedo, True, start=s)[first - s:first - s + count]
        assert len(got) == count and all(same(g, w) for g, w in zip(got, want)), (warmup, feedback)
        whole = chain(ctx, np.float32, True, feedback, np.float32, albedo, True)[first:first + count]
        assert all(same(g, w) for g, w in zip(got, whole)) == (s == 0), warmup


@pytest.mark.parametrize("albedo", (False, True), ids=("colour", "illumination"))
@pytest.mark.parametrize("odt", (np.uint8, np.float16, np.float32), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("pinned_out", (False, True), ids=("pageable", "pinned"))
def test_output_formats_and_host_memory_kinds(ctx, pinned_out, odt, albedo):
    """Without albedo and firefly the box is taken from the frame in the frames' own format: u8, f16, f32."""
    fdt = np.uint8 if odt == np.uint8 else np.float16 if odt == np.float16 else np.float32
    want = chain(ctx, fdt, True, 1, odt, albedo, False)
    for pinned in (False, True):
        got = run(ctx, fdt, True, 1, odt, albedo, False, pinned=pinned, pinned_out=pinned_out, first=2, count=5, warmup=4)
        assert all(g.dtype == np.dtype(odt) and same(g, w) for g, w in zip(got, want[2:7])), (pinned, pinned_out)


def test_no_clip_is_the_firefly_entry_point(ctx):
    fr = frames_of()
    kw = dict(motion=MOTION, feedback=1, passes=PASSES, **ACC, **VAR)
    for alb in (None, ALBEDO):
        for ff in ({}, FFKW):
            plain, _ = ctx.sequence_atrous_recursive(fr, LAYERS, SG, albedo=alb, albedo_floor=FLOOR, **ff, **kw)
            off, _ = ctx.sequence_atrous_recursive(fr, LAYERS, SG, albedo=alb, albedo_floor=FLOOR, clip_gamma=None, **ff, **kw)
            assert all(same(a, b) for a, b in zip(plain, off))
    # and cp == NULL through the new entry point itself
    h, w = SHAPE
    flat = [l for ls in LAYERS for l in ls]
    outs = [[np.zeros((h, w, 4), np.float32) for _ in range(N)] for _ in range(2)]
    ap = mid.TemporalAccumParams(w, h, 0.2, 0.25, 6, 3, mid.FMT_RGBA32F)
    vp = mid.AtrousVarianceParams(w, h, 0, PASSES, 4.0, 1e-3, mid.FMT_RGBA32F)
    fp = mid.FireflyParams(w, h, FF["radius"], FF["rank"], FF["gain"], FF["floor"], mid.FMT_RGBA32F)
    sg = (ctypes.c_float * L)(*SG)
    head = (ctx.handle, ctypes.byref(ap), ctypes.byref(vp), sg, (ctypes.c_void_p * N)(*[a.ctypes.data for a in fr]), N,
            (ctypes.c_void_p * len(flat))(*[a.ctypes.data for a in flat]), L, None, None, 0.0, ctypes.byref(fp))
    tail = lambda o: (1, 16, 0, N, (ctypes.c_void_p * N)(*[a.ctypes.data for a in o]), mid.FMT_RGBA32F, 1, (ctypes.c_float * 3)())
    assert mid.lib.mid_sequence_atrous_recursive_clip(*head, None, *tail(outs[0])) == 0, mid.lib.mid_last_error()
    assert mid.lib.mid_sequence_atrous_recursive_firefly(*head, *tail(outs[1])) == 0, mid.lib.mid_last_error()
    assert all(same(a, b) for a, b in zip(*outs)) and all(np.isfinite(a).all() and a.any() for a in outs[0])


# ---- the demonstration ---------------------------------------------------------------------------------------------------------

def test_a_light_that_switches_leaves_no_ghost(ctx):
    """Noise-free grey frames of B with a 32 x 32 square of A, one constant layer, zero motion, alpha 0.2, one pass; at frame 6 the square
    turns to B.  With the clip the output of frame 6 at the square's centre is B to 1e-5 max(1, B): the box of a constant
    neighbourhood is [B, B], so the history is replaced.  Without it the output is within 1e-5 of A + 0.2 (B - A): N' = 7 there, so
    the blend factor is alpha.  tests/test_history_clip_args.py derives both numbers with the checkers."""
    frames, layers = hci.demo_frames()
    A, B = hci.DEMO_A, hci.DEMO_B
    y, x = hci.DEMO_CENTRE
    kw = dict(feedback=1, passes=1, alpha=0.2, alpha_moments=0.2, history_max=32, history_full=4, sigma_lum=4.0)
    with_clip = ctx.sequence_atrous_recursive(frames, layers, [0.1], clip_gamma=1.0, **kw)[0]
    without = ctx.sequence_atrous_recursive(frames, layers, [0.1], **kw)[0]
    t6 = hci.DEMO_SWITCH
    for o in (with_clip, without):
        assert np.abs(o[t6 - 1][y, x, :3].astype(np.float64) - A).max() <= 1e-5       # before the switch both show A
    got, ghost = with_clip[t6][y, x, :3].astype(np.float64), without[t6][y, x, :3].astype(np.float64)
    print(f"frame {t6} at the square's centre: with the clip {got}, without {ghost}; B = {B}, A + 0.2 (B - A) = {A + 0.2 * (B - A)}")
    assert np.abs(got - B).max() <= 1e-5 * max(1.0, B)
    assert np.abs(ghost - (A + 0.2 * (B - A))).max() <= 1e-5
    assert np.abs(with_clip[t6][..., :3].astype(np.float64) - B).max() <= 1e-5       # the whole frame is the new lighting


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(ctx):
    fr = frames_of()
    h, w = SHAPE
    flat = [l for ls in LAYERS for l in ls]
    outs = [np.full((h, w, 4), 7.0, np.float32) for _ in range(N)]
    hin, hl, hout = ([a.ctypes.data for a in arrs] for arrs in (fr, flat, outs))
    ap = mid.TemporalAccumParams(w, h, 0.2, 0.25, 6, 3, mid.FMT_RGBA32F)
    vp = mid.AtrousVarianceParams(w, h, 0, PASSES, 4.0, 1e-3, mid.FMT_RGBA32F)
    sg = (ctypes.c_float * L)(*SG)

    def call(cp, feedback=1):
        t = (ctypes.c_float * 3)()
        return mid.lib.mid_sequence_atrous_recursive_clip(ctx.handle, ctypes.byref(ap), ctypes.byref(vp), sg, (ctypes.c_void_p * N)(*hin), N,
                                                          (ctypes.c_void_p * len(hl))(*hl), L, None, None, 0.0, None, ctypes.byref(cp), feedback, 16, 0, N,
                                                          (ctypes.c_void_p * N)(*hout), mid.FMT_RGBA32F, 1, t)

    def refused(*words, feedback=1, **kw):
        args = dict(width=w, height=h, radius=1, gamma=1.0, format=mid.FMT_RGBA32F)
        args.update(kw)
        rc = call(mid.ColorBoundsParams(*[args[k] for k in ("width", "height", "radius", "gamma", "format")]), feedback)
        msg = mid.lib.mid_last_error().decode()
        assert rc == 1 and all(x in msg for x in words) and "sequence_atrous_recursive_clip" in msg, (rc, msg)
        assert all((o == 7.0).all() for o in outs), "an output was touched"

    refused(f"{w + 1}x{h}", f"{w}x{h}", width=w + 1)
    refused(f"{w}x{h - 1}", f"{w}x{h}", height=h - 1)
    refused("0x1", "format 0", format=mid.FMT_RGBA8)                       # the frames are RGBA32F: both values are named
    refused("guide bits", format=mid.FMT_RGBA32F | (3 << 8))
    refused("radius", radius=3)
    refused("radius", radius=0)
    refused("gamma", gamma=-1.0)
    refused("gamma", gamma=float("nan"))
    refused("gamma", gamma=float("inf"))
    refused("feedback", feedback=2)                                        # (and a refusal of the existing call, under the new name)
    # and the valid call still runs into these buffers
    assert call(mid.ColorBoundsParams(w, h, CLIP["radius"], CLIP["gamma"], mid.FMT_RGBA32F)) == 0, mid.lib.mid_last_error()
    want = chain(ctx, np.float32, False, 1, np.float32, False, False)
    assert all(same(o, c) for o, c in zip(outs, want))
