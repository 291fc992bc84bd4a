"""The packed right-edge shape of the NLM strip kernel on the GPU (csrc/nlm_edge.hip): a LONG k = 0 launch of a tuned window covers the
ragged last tile column with workgroups of four tiles each, beside a main launch that leaves the column out -- and every pixel keeps the
bits the whole shape gives it.

A launch is long from kNlmSmallRounds * 2 * CUs workgroups on, and one launch takes at most 96 frames, so the frames here are as small
as a long launch allows: five tile rows (h = 150: one full group of four tiles, one group with a single live tile, a ragged last tile)
by as many tile columns as make 96 frames long -- 8 at 256 CUs -- of which the last holds the most columns that still pack (6 at the 7x7
patch, 7 at 6x6).  The frames the rule was stated with, two tile columns wide (122 = 2 x 58 + 6; 124: 8 valid columns, not packed; 116: no
ragged column), run through the same comparisons; at 256 CUs their 96 x 15 workgroups are a small launch, which nlm_small.hip keeps whole.

The reference bits are each frame filtered ALONE: a launch of a few workgroups, which nlm_small.hip runs unpacked.
"""
import functools

import numpy as np
import pytest
import torch

import image_denoising_filter_amd as mid
import np_reference
import opaque_vote_cases as ov
from conftest import rel_err
from opaque_vote_cases import NLM_TOL

pytestmark = pytest.mark.gpu

H, N_FRAMES, N_DISTINCT = 150, 96, 4
DTYPES = {"f32": np.float32, "u8": np.uint8, "f16": np.float16}


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def geometry(window):
    search, patch = ov.NLM_WINDOWS[window]
    pw = patch[1] - patch[0]
    return search, patch, pw, 64 - (pw - 1), 12 - (pw - 1)        # ..., VW, the most valid columns that pack


def width(window, kind, cols):
    _, _, pw, vw, most = geometry(window)
    n = 2 if cols == "two" else next(c for c in range(2, 64) if c * -(-H // 32) * N_FRAMES > ov.NLM_SMALL_ROUNDS * 2 * cu_count())
    return {"packed": (n - 1) * vw + most, "wider": (n - 1) * vw + most + 2, "even": n * vw}[kind]


@functools.lru_cache(None)
def frames_of(w, dtype_name):
    """N_DISTINCT frames: smooth colour + noise; frames 1 and 3 carry translucent texels, most of them in the last columns."""
    rng = np.random.default_rng(w * 7 + len(dtype_name))
    yy, xx = np.mgrid[0:H, 0:w].astype(np.float32)
    out = []
    for i in range(N_DISTINCT):
        rgb = np.stack([0.5 + 0.3 * np.sin(xx * 0.21 + i), 0.5 + 0.3 * np.cos(yy * 0.17 - i), (xx + 2 * yy) / (w + 2 * H)], -1)
        rgb = rgb + rng.normal(0, 0.04, rgb.shape)
        a = np.ones((H, w, 1))
        if i % 2:
            a[rng.random((H, w, 1)) < 0.01] = 0.25
            a[:, -20:][rng.random((H, 20, 1)) < 0.3] = 0.5
        img = np.concatenate([np.clip(rgb, 0, 1), a], -1)
        out.append((img * 255).astype(np.uint8) if dtype_name == "u8" else img.astype(DTYPES[dtype_name]))
    return out


def batched(ctx, frames, window, stream_body=None):
    """N_FRAMES outputs of one k = 0 launch over frames[i % N_DISTINCT] (inputs may alias)."""
    h, w = frames[0].shape[:2]
    search, patch = ov.NLM_WINDOWS[window]
    d_in = [ctx.upload(f) for f in frames]
    d_out = [ctx.zeros(h * w * 16) for _ in range(N_FRAMES)]
    ctx.sync()
    fmt = {np.dtype(np.float32): mid.FMT_RGBA32F, np.dtype(np.uint8): mid.FMT_RGBA8, np.dtype(np.float16): mid.FMT_RGBA16F}[frames[0].dtype]
    call = lambda: ctx.nlm_temporal_dev([d_in[i % N_DISTINCT].ptr for i in range(N_FRAMES)], [d.ptr for d in d_out], w, h, ov.HPARAM,
                                        search, patch, 0, 0, N_FRAMES, fmt)
    if stream_body is None:
        call()
    else:
        stream_body(call)
    ctx.sync()
    return [ctx.download(d, (h, w, 4), np.float32) for d in d_out]


def alone(ctx, frames, window):
    search, patch = ov.NLM_WINDOWS[window]
    return [ctx.nlm_temporal([f], k=0, hparam=ov.HPARAM, search=search, patch=patch)[0] for f in frames]


def check_batch(outs, refs, label):
    for i, o in enumerate(outs):
        r = refs[i % N_DISTINCT]
        assert np.array_equal(o, r), f"{label}: output {i} differs from its frame filtered alone in {int(np.sum(np.any(o != r, -1)))} pixels, " \
                                     f"columns {sorted(set(np.nonzero(np.any(o != r, -1))[1]))[:8]}"


CASES = [("long", d) for d in DTYPES] + [("two", "f32")]


@pytest.mark.parametrize("cols,dtype_name", CASES)
@pytest.mark.parametrize("kind", ["packed", "wider", "even"])
@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
def test_batched_launch_is_each_frame_alone(ctx, window, kind, cols, dtype_name):
    w = width(window, kind, cols)
    frames = frames_of(w, dtype_name)
    refs = alone(ctx, frames, window)
    assert not any(np.array_equal(refs[0], r) for r in refs[1:]) and all(np.isfinite(r).all() for r in refs)
    assert np.any(refs[1][:, -3:, 3] != 1.0), "translucent texels show in the last columns"
    check_batch(batched(ctx, frames, window), refs, f"{window} {kind} w={w} {dtype_name}")


@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
def test_packed_columns_against_the_float64_reference(ctx, window):
    """np_reference.nlm_sums on the last 46 columns of one frame of the batch (the frame's own right edge; the 13 columns next to the cut
    see texels the crop lacks and are left out): the packed columns and the main launch's last ones."""
    search, patch, pw, vw, most = geometry(window)
    w = width(window, "packed", "long")
    frames = frames_of(w, "f32")
    outs = batched(ctx, frames, window)
    reach = max(-search[0], search[1] - 1) + max(-patch[0], patch[1] - 1)
    crop = frames[1][:, w - 46:]
    num, den = np_reference.nlm_sums(crop, crop, ov.HPARAM, search, patch)
    want = (num / den[..., None])[:, reach:]
    got = outs[N_DISTINCT + 1][:, w - 46 + reach:]
    assert want.shape[1] > most + 20
    err = rel_err(got, want)
    print(f"packed edge {window}: rel err {err:.3g} over the last {want.shape[1]} columns")
    assert err < NLM_TOL


@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
def test_recorded_call_gives_the_by_call_bits(ctx, window):
    """While the stream records the launch stays whole -- one kernel node -- and the submitted recording writes the bits of the call."""
    w = width(window, "packed", "long")
    frames = frames_of(w, "f32")
    by_call = batched(ctx, frames, window)
    seen = {}

    def recorded(call):
        with ctx.record(None) as rec:
            call()
        seen["info"] = rec.info()
        rec.submit(None)
        ctx.sync()
        rec.close()

    outs = batched(ctx, frames, window, recorded)
    assert seen["info"][1] == 1, seen
    for a, b in zip(outs, by_call):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("window", list(ov.NLM_WINDOWS))
def test_nlm_accum_packed_against_unpacked(ctx, window):
    """mid_nlm_accum is one frame a launch, so a long one is a TALL frame: three tile columns (the last one packed) by enough tile rows,
    ragged at the bottom.  The unpacked bits of its last columns come from 150-row crops at strip-aligned rows -- a pixel's bits depend on its
    row within the strip and on the texels in reach, and an edge tile runs the general form in either launch -- with the 13 rows next to
    a cut left out."""
    search, patch, pw, vw, most = geometry(window)
    w = 2 * vw + most
    tiles_y = ov.NLM_SMALL_ROUNDS * 2 * cu_count() // 3 + 1
    h = tiles_y * 32 - 10
    assert ov.nlm_tile_workgroups(w, h, pw, 1) > ov.NLM_SMALL_ROUNDS * 2 * cu_count()
    rng = np.random.default_rng(11)
    yy = np.arange(h, dtype=np.float32)[:, None, None]
    xx = np.arange(w, dtype=np.float32)[None, :, None]
    base = 0.5 + 0.3 * np.sin(xx * 0.2 + yy * 0.013 + np.arange(3, dtype=np.float32))
    tgt = np.concatenate([base + rng.normal(0, 0.04, (h, w, 3)).astype(np.float32), np.ones((h, w, 1), np.float32)], -1).astype(np.float32)
    nb = tgt.copy()
    nb[..., :3] += rng.normal(0, 0.04, (h, w, 3)).astype(np.float32)
    nb[..., 3][rng.random((h, w)) < 0.05] = 0.5
    W0 = rng.random((h, w, 8), dtype=np.float32)
    W = ctx.nlm_accum(tgt, nb, W0, ov.HPARAM, search, patch)
    reach = max(-search[0], search[1] - 1) + max(-patch[0], patch[1] - 1)
    checked = 0
    for r0 in (0, 32 * (tiles_y // 2), 32 * (tiles_y - 4)):
        r1 = min(r0 + 150, h)
        Wc = ctx.nlm_accum(tgt[r0:r1], nb[r0:r1], W0[r0:r1], ov.HPARAM, search, patch)
        lo = 0 if r0 == 0 else reach
        hi = r1 - r0 if r1 == h else r1 - r0 - reach
        a, b = W[r0 + lo:r0 + hi, w - most:], Wc[lo:hi, w - most:]
        assert not np.array_equal(b, W0[r0 + lo:r0 + hi, w - most:])
        assert np.array_equal(a, b), f"nlm_accum {window}: rows {r0 + lo}..{r0 + hi} differ in {int(np.sum(np.any(a != b, -1)))} pixels"
        checked += a.shape[0]
    assert checked > 300
    assert np.all(W[..., :5] != W0[..., :5]), "every pixel was accumulated once"
