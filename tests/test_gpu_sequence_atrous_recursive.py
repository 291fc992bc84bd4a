"""GPU suite: the recursive temporal accumulation as a stage of the frame pipeline (mid_sequence_atrous_recursive, section a4j).

Eight frames of 131 x 67, two passes.  Every output must equal, BIT FOR BIT, the chain of public calls started at frame
s = max(0, first - warmup): atrous_moments at k = 0, temporal_accumulate with the previous step's history, atrous_variance -- for
both feedback values (the next colour history is the accumulated colour, or the level after pass 0), with and without motion
planes, with overlap 0 and 1, for pageable and page-locked outputs and u8 / f16 / f32 outputs.  A sub-range with warm-up equals the
call on the frames from s on, and the whole run when the warm-up reaches frame 0.  Refusals leave host_out untouched.
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


def frames_of(dt=np.float32):
    return [tai.frame_of(SHAPE, t, dt) for t in range(N)]


LAYERS = [tai.layers_of(SHAPE, L, np.uint8, t) for t in range(N)]
MOTION = [np.roll(tai.motion_of(SHAPE, "smooth"), 5 * t, 1) * np.float32(0.5 + 0.1 * t) for t in range(N)]
CHAINS = {}


def chain(ctx, fdt, with_motion, feedback, odt, start=0):
    """The outputs of frames start .. N-1 by public calls, the history starting at frame `start`."""
    key = (np.dtype(fdt).name, with_motion, feedback, np.dtype(odt).name, start)
    if key not in CHAINS:
        fr, hist, outs = frames_of(fdt), None, []
        for t in range(start, N):
            vs = ctx.atrous_moments([fr[t]], [LAYERS[t]], SG, k=0, t=0)
            col, st, var = ctx.temporal_accumulate(fr[t], LAYERS[t], LAYERS[t - 1] if hist is not None else LAYERS[t], SG, hist=hist,
                                                   motion=MOTION[t] if with_motion else None, var_spatial=vs, **ACC)
            if feedback == 0:
                outs.append(ctx.atrous_variance(col, var, LAYERS[t], SG, passes=PASSES, out_dtype=odt, **VAR))
                hist = (col, st)
            else:
                lvl, v1 = ctx.atrous_variance(col, var, LAYERS[t], SG, passes=1, return_variance=True, **VAR)
                outs.append(ctx.atrous_variance(lvl, v1, LAYERS[t], SG, passes=PASSES - 1, first_pass=1, out_dtype=odt, **VAR))
                hist = (lvl, st)
        CHAINS[key] = outs
    return CHAINS[key]


def run(ctx, fdt, with_motion, feedback, odt, frames=slice(None), **kw):
    fr = frames_of(fdt)[frames]
    outs, _ = ctx.sequence_atrous_recursive(fr, LAYERS[frames], SG, motion=MOTION[frames] if with_motion else None, feedback=feedback, passes=PASSES,
                                            out_dtype=odt, **ACC, **VAR, **kw)
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


@pytest.mark.parametrize("feedback", (0, 1))
@pytest.mark.parametrize("warmup", (0, 2, 8))
def test_a_sub_range_with_warm_up(ctx, warmup, feedback):
    first, count = 3, 2
    s = max(0, first - warmup)
    got = run(ctx, np.float32, True, feedback, np.float32, first=first, count=count, warmup=warmup)
    want = chain(ctx, np.float32, True, feedback, np.float32, start=s)[first - s:first - s + count]
    assert len(got) == count and all(same(g, w) for g, w in zip(got, want)), (warmup, feedback)
    # ... which is the call on frames[s:] ...
    cut = run(ctx, np.float32, True, feedback, np.float32, frames=slice(s, None), first=first - s, count=count, warmup=warmup)
    assert all(same(g, c) for g, c in zip(got, cut))
    # ... and the whole run when the warm-up reaches frame 0 -- and only then
    whole = chain(ctx, np.float32, True, feedback, np.float32)[first:first + count]
    assert all(same(g, w) for g, w in zip(got, whole)) == (s == 0), warmup


@pytest.mark.parametrize("odt", (np.uint8, np.float16, np.float32), ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("pinned_out", (False, True), ids=("pageable", "pinned"))
def test_output_formats_and_host_memory_kinds(ctx, pinned_out, odt):
    fdt = np.uint8 if odt == np.uint8 else np.float32
    want = chain(ctx, fdt, True, 1, odt)
    for pinned in (False, True):
        got = run(ctx, fdt, True, 1, odt, pinned=pinned, pinned_out=pinned_out, first=2, count=5, warmup=4)
        assert all(g.dtype == np.dtype(odt) and same(g, w) for g, w in zip(got, want[2:7])), (pinned, pinned_out)


def test_refusals_leave_the_outputs_untouched(ctx):
    fr = frames_of()
    h, w = SHAPE
    flat = [l for ls in LAYERS for l in ls]
    outs = [np.full((h, w, 4), 7.0, np.float32) for _ in range(N)]
    hin, hl, hmv, hout = ([a.ctypes.data for a in arrs] for arrs in (fr, flat, MOTION, outs))

    def refused(word, hin=hin, hl=hl, hmv=hmv, hout=hout, n_layers=L, sigmas=SG, **kw):
        with pytest.raises(mid.MidError) as e:
            ctx.sequence_atrous_recursive_pinned(hin, hout, w, h, mid.FMT_RGBA32F, hl, n_layers, sigmas, hmv, **dict(dict(passes=PASSES, **ACC, **VAR), **kw))
        assert word in str(e.value), str(e.value)
        assert all((o == 7.0).all() for o in outs), "an output was touched"

    refused("feedback", feedback=2)
    refused("feedback", feedback=-1)
    refused("warmup", warmup=-1)
    refused("alpha ", alpha=0.0)
    refused("alphaMoments", alpha_moments=1.5)
    refused("historyMax", history_max=0.5)
    refused("historyFull", history_full=1.0)
    refused("sigmaLum", sigma_lum=-1.0)
    refused("epsilon", epsilon=0.0)
    refused("passes", passes=9)
    refused("sigmas must be finite", sigmas=[0.1, 0.0, 0.1])
    refused("bad range", first=7, count=2)
    refused("bad range", count=0)
    refused("frame 1 is NULL", hin=[hin[0], None] + hin[2:], first=3, count=2, warmup=2)          # a warm-up frame
    refused("layer 1 of frame 2 is NULL", hl=hl[:2 * L + 1] + [None] + hl[2 * L + 2:])
    refused("motion plane of frame 4 is NULL", hmv=hmv[:4] + [None] + hmv[5:])
    refused("output 1 is NULL", hout=[hout[0], None] + hout[2:])
    refused("is also", hout=[hin[3]] + hout[1:])
    refused("is also", hout=[hmv[2]] + hout[1:])
    refused("appears twice", hout=[hout[0], hout[0]] + hout[2:])
    with pytest.raises(mid.MidError):                        # vp->first_pass != 0, through the raw call
        import ctypes
        ap = mid.TemporalAccumParams(w, h, 0.2, 0.2, 32.0, 4.0, mid.FMT_RGBA32F)
        vp = mid.AtrousVarianceParams(w, h, 1, 2, 4.0, 1e-3, mid.FMT_RGBA32F)
        rc = mid.lib.mid_sequence_atrous_recursive(ctx.handle, ctypes.byref(ap), ctypes.byref(vp), (ctypes.c_float * L)(*SG), (ctypes.c_void_p * N)(*hin), N,
                                                   (ctypes.c_void_p * len(hl))(*hl), L, None, 1, 0, 0, N, (ctypes.c_void_p * N)(*hout), mid.FMT_RGBA32F, 1, None)
        assert rc == 1 and b"first_pass" in mid.lib.mid_last_error()
        raise mid.MidError(rc, "mid_sequence_atrous_recursive")
    assert all((o == 7.0).all() for o in outs)
    # and the valid call still runs into these buffers
    ctx.sequence_atrous_recursive_pinned(hin, hout, w, h, mid.FMT_RGBA32F, hl, L, SG, hmv, passes=PASSES, **ACC, **VAR)
    assert all(same(o, c) for o, c in zip(outs, chain(ctx, np.float32, True, 1, np.float32)))
