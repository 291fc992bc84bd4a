"""GPU suite: the recursive a-trous sequence on ILLUMINATION (mid_sequence_atrous_recursive_albedo, section a4k).

Eight frames of 131 x 67 from tests/temporal_accumulate_inputs.py, two passes; the albedo of frame t is a one-pixel checker of 0.2 / 0.8
(shifted by t) with a few zero texels, in the layers' format.  Every output must equal, BIT FOR BIT, the chain of public calls
demodulate -> atrous_moments -> temporal_accumulate -> atrous_variance (float32 out) -> modulate: both feedback values, with and
without motion, overlap 0 and 1, pageable and page-locked outputs, u8 / f16 / f32 outputs, sub-ranges with warm-up.  albedo=None and
an all-ones albedo give the bits of the existing call.  Refusals leave host_out untouched.  And the point of it all, with numbers
that can be derived: a textured frame c * A keeps its texture with the albedo and loses it without.
"""
import numpy as np
import pytest

import image_denoising_filter_amd as mid
import temporal_accumulate_inputs as tai
from test_gpu_atrous_bounds import same

pytestmark = pytest.mark.gpu

SHAPE, N, L, PASSES = (67, 131), 8, 3, 2
SG = tai.sigmas_of(L)
ACC = dict(alpha=0.2, alpha_moments=0.25, history_max=6, history_full=3)
VAR = dict(sigma_lum=4.0, epsilon=1e-3)
FLOOR = 2e-3


def checker(t, dt=np.uint8, zeros=True):
    """0.2 / 0.8 in squares of one pixel, shifted by t; uint8 planes hold the codes 51 / 204."""
    h, w = SHAPE
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.where((xx + yy + t) % 2 == 0, 0.2, 0.8)
    a = np.repeat(a[..., None], 4, -1)
    a[..., 1] = np.where((xx + yy + t) % 2 == 0, 0.8, 0.2)              # (green carries the opposite phase)
    if zeros:
        a[3 + t, 5:9, :3] = 0.0
        a[40, 100 + t, 0] = 0.0
    return np.round(a * 255).astype(np.uint8) if np.dtype(dt) == np.uint8 else a.astype(dt)


def frames_of(dt=np.float32):
    return [tai.frame_of(SHAPE, t, dt) for t in range(N)]


LAYERS = [tai.layers_of(SHAPE, L, np.uint8, t) for t in range(N)]
ALBEDO = [checker(t) for t in range(N)]
MOTION = [np.roll(tai.motion_of(SHAPE, "smooth"), 5 * t, 1) * np.float32(0.5 + 0.1 * t) for t in range(N)]
CHAINS = {}


def chain(ctx, fdt, with_motion, feedback, odt, start=0):
    """The outputs of frames start .. N-1 by public calls on the illumination, the history starting at frame `start`."""
    key = (np.dtype(fdt).name, with_motion, feedback, np.dtype(odt).name, start)
    if key not in CHAINS:
        fr, hist, outs = frames_of(fdt), None, []
        for t in range(start, N):
            il = ctx.demodulate(fr[t], ALBEDO[t], FLOOR)
            vs = ctx.atrous_moments([il], [LAYERS[t]], SG, k=0, t=0)
            col, st, var = ctx.temporal_accumulate(il, LAYERS[t], LAYERS[t - 1] if hist is not None else LAYERS[t], SG, hist=hist,
                                                   motion=MOTION[t] if with_motion else None, var_spatial=vs, **ACC)
            if feedback == 0:
                fin = ctx.atrous_variance(col, var, LAYERS[t], SG, passes=PASSES, **VAR)
                hist = (col, st)
            else:
                lvl, v1 = ctx.atrous_variance(col, var, LAYERS[t], SG, passes=1, return_variance=True, **VAR)
                fin = ctx.atrous_variance(lvl, v1, LAYERS[t], SG, passes=PASSES - 1, first_pass=1, **VAR)
                hist = (lvl, st)
            assert fin.dtype == np.float32
            outs.append(ctx.modulate(fin, ALBEDO[t], FLOOR, out_dtype=odt))
        CHAINS[key] = outs
    return CHAINS[key]


def run(ctx, fdt, with_motion, feedback, odt, frames=slice(None), albedo=ALBEDO, floor=FLOOR, **kw):
    fr = frames_of(fdt)[frames]
    outs, _ = ctx.sequence_atrous_recursive(fr, LAYERS[frames], SG, motion=MOTION[frames] if with_motion else None, feedback=feedback, passes=PASSES,
                                            out_dtype=odt, albedo=None if albedo is None else albedo[frames], albedo_floor=floor, **ACC, **VAR, **kw)
    return outs


@pytest.mark.parametrize("feedback", (0, 1))
@pytest.mark.parametrize("with_motion", (False, True), ids=("still", "motion"))
def test_every_output_is_the_chain_of_public_calls(ctx, with_motion, feedback):
    want = chain(ctx, np.float32, with_motion, feedback, np.float32)
    for overlap in (1, 0):
        got = run(ctx, np.float32, with_motion, feedback, np.float32, overlap=bool(overlap))
        assert len(got) == N and all(same(g, w) for g, w in zip(got, want)), (with_motion, feedback, overlap)
    assert not same(want[-1], chain(ctx, np.float32, not with_motion, feedback, np.float32)[-1])       # (the motion planes matter)
    assert not same(want[-1], chain(ctx, np.float32, with_motion, 1 - feedback, np.float32)[-1])        # (and so does the feedback)
    assert not same(want[-1], run(ctx, np.float32, with_motion, feedback, np.float32, albedo=None)[-1])  # (and the albedo)
    assert not same(want[-1], run(ctx, np.float32, with_motion, feedback, np.float32, floor=0.3)[-1])    # (and its floor)


@pytest.mark.parametrize("feedback", (0, 1))
@pytest.mark.parametrize("warmup", (0, 2, 8))
def test_a_sub_range_with_warm_up(ctx, warmup, feedback):
    first, count = 3, 2
    s = max(0, first - warmup)
    got = run(ctx, np.float32, True, feedback, np.float32, first=first, count=count, warmup=warmup)
    want = chain(ctx, np.float32, True, feedback, np.float32, start=s)[first - s:first - s + count]
    assert len(got) == count and all(same(g, w) for g, w in zip(got, want)), (warmup, feedback)
    whole = chain(ctx, np.float32, True, feedback, np.float32)[first:first + count]
    assert all(same(g, w) for g, w in zip(got, whole)) == (s == 0), warmup


@pytest.mark.parametrize("odt", (np.uint8, np.float16, np.float32), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("pinned_out", (False, True), ids=("pageable", "pinned"))
def test_output_formats_and_host_memory_kinds(ctx, pinned_out, odt):
    fdt = np.uint8 if odt == np.uint8 else np.float16 if odt == np.float16 else np.float32
    want = chain(ctx, fdt, True, 1, odt)
    for pinned in (False, True):
        got = run(ctx, fdt, True, 1, odt, pinned=pinned, pinned_out=pinned_out, first=2, count=5, warmup=4)
        assert all(g.dtype == np.dtype(odt) and same(g, w) for g, w in zip(got, want[2:7])), (pinned, pinned_out)


def test_no_albedo_and_an_albedo_of_ones_are_the_existing_call(ctx):
    fr = frames_of()
    layers = [tai.layers_of(SHAPE, L, np.float32, t) for t in range(N)]
    kw = dict(motion=MOTION, feedback=1, passes=PASSES, **ACC, **VAR)
    plain, _ = ctx.sequence_atrous_recursive(fr, layers, SG, **kw)
    none, _ = ctx.sequence_atrous_recursive(fr, layers, SG, albedo=None, albedo_floor=0.5, **kw)
    ones, _ = ctx.sequence_atrous_recursive(fr, layers, SG, albedo=[np.ones(SHAPE + (4,), np.float32)] * N, **kw)
    assert all(same(a, b) for a, b in zip(plain, none))
    assert all(same(a, b) for a, b in zip(plain, ones))                  # division and product by 1 are exact
    half, _ = ctx.sequence_atrous_recursive(fr, layers, SG, albedo=[np.full(SHAPE + (4,), 0.3, np.float32)] * N, **kw)
    assert not same(plain[-1], half[-1])                                 # (any other albedo rounds twice and scales the luminance the variance sees)
    with pytest.raises(ValueError):                                      # the albedo obeys the layers' format
        ctx.sequence_atrous_recursive(fr, layers, SG, albedo=ALBEDO, **kw)


def test_refusals_leave_the_outputs_untouched(ctx):
    fr = frames_of()
    h, w = SHAPE
    flat = [l for ls in LAYERS for l in ls]
    outs = [np.full((h, w, 4), 7.0, np.float32) for _ in range(N)]
    hin, hl, hmv, hal, hout = ([a.ctypes.data for a in arrs] for arrs in (fr, flat, MOTION, ALBEDO, outs))

    def refused(word, hal=hal, hout=hout, **kw):
        with pytest.raises(mid.MidError) as e:
            ctx.sequence_atrous_recursive_pinned(hin, hout, w, h, mid.FMT_RGBA32F, hl, L, SG, hmv, halbedo=hal, **dict(dict(passes=PASSES, albedo_floor=FLOOR, **ACC, **VAR), **kw))
        assert word in str(e.value), str(e.value)
        assert all((o == 7.0).all() for o in outs), "an output was touched"

    refused("albedo plane of frame 4 is NULL", hal=hal[:4] + [None] + hal[5:])
    refused("albedo plane of frame 1 is NULL", hal=[hal[0], None] + hal[2:], first=3, count=2, warmup=2)      # a warm-up frame
    refused("is also", hout=[hal[2]] + hout[1:])
    refused("is also", hout=hout[:6] + [hal[7], hout[7]])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("floor", albedo_floor=bad)
    refused("feedback", feedback=2)                                      # (the existing refusals still come first or after: all are refusals)
    with pytest.raises(ValueError):
        ctx.sequence_atrous_recursive_pinned(hin, hout, w, h, mid.FMT_RGBA32F, hl, L, SG, hmv, halbedo=hal[:3], passes=PASSES, **ACC, **VAR)
    assert all((o == 7.0).all() for o in outs)
    # and the valid call still runs into these buffers
    ctx.sequence_atrous_recursive_pinned(hin, hout, w, h, mid.FMT_RGBA32F, hl, L, SG, hmv, halbedo=hal, albedo_floor=FLOOR, passes=PASSES, **ACC, **VAR)
    assert all(same(o, c) for o, c in zip(outs, chain(ctx, np.float32, True, 1, np.float32)))


def test_the_texture_survives(ctx):
    """Frames c * A with a constant c and the one-pixel checker A, one constant guide layer, sigma_lum = 0: every weight is the B3
    kernel's, the passes are a plain blur reaching +-62 pixels.
    With the albedo the illumination fl(c A) / A is c up to one rounding, a weighted mean and a lerp of values within an ulp of c
    stay within a few ulp of c, and the product with A is the frame up to a few parts in 2^24: within 1e-5 max(1, |frame|).
    Without it the blur mixes 0.2 c and 0.8 c towards 0.5 c: 0.3 c = 0.21 away from the frame in the red channel."""
    n, h, w = 3, SHAPE[0], SHAPE[1]
    c = np.float32([0.7, 0.5, 0.3, 1.0])
    A = [checker(t, np.float32, zeros=False) for t in range(n)]
    fr = []
    for a in A:
        f = (c * a).astype(np.float32)
        f[..., 3] = 1.0
        fr.append(f)
    layers = [[np.full((h, w, 4), 0.5, np.float32)] for _ in range(n)]
    kw = dict(passes=5, sigma_lum=0.0)
    with_albedo, _ = ctx.sequence_atrous_recursive(fr, layers, [0.1], albedo=A, **kw)
    without, _ = ctx.sequence_atrous_recursive(fr, layers, [0.1], **kw)
    for t in range(n):
        err = np.abs(with_albedo[t].astype(np.float64) - fr[t]) / np.maximum(1.0, np.abs(fr[t]))
        print(f"frame {t}: with the albedo {err.max():.3e} from the frame, without {np.abs(without[t] - fr[t]).max():.3f}")
        assert err.max() <= 1e-5, t
        assert np.abs(without[t] - fr[t]).max() > 0.1, t
