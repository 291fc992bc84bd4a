"""GPU suite: layer-guided NLM over neighbouring frames through the frame pipeline (mid_sequence_nlm_layers_temporal) -- output t has
the bits of the resident mid_nlm_layers_temporal, for the three output formats, with and without overlap, page-locked and pageable
host memory, more frames than the ring holds, sub-ranges with halo, and two frame blocks against the whole sequence."""
import ctypes

import numpy as np
import pytest

import image_denoising_filter_amd as mid
from test_gpu_sequence_nlm_layers import CFG, H, OUT, _direct, assert_same, frames_of, layers_of

pytestmark = pytest.mark.gpu


def resident(ctx, frames, layers, k, out_dt, cfg, first=0, count=None):
    return ctx.nlm_layers_temporal(frames, layers, k, first, count, hparam=H, out_dtype=out_dt, **CFG[cfg])


@pytest.mark.parametrize("in_dt", [np.float32, np.uint8, np.float16])
def test_more_frames_than_the_ring_every_output_format_and_host_memory(ctx, in_dt):
    rng = np.random.default_rng(41)
    h, w, n, k = 48, 100, 12, 2                      # n >= 2k + 6: ring slots are reused while later outputs still read their neighbours
    frames = frames_of(rng, n, h, w, in_dt)
    layers = layers_of(rng, n, 2, h, w)
    for out_dt in OUT:
        want = resident(ctx, frames, layers, k, out_dt, "bench")
        for pinned in (True, False):
            for overlap in (True, False):
                got, t = ctx.sequence_nlm_layers_temporal(frames, layers, k, overlap=overlap, hparam=H, pinned=pinned,
                                                          pinned_out=pinned, out_dtype=out_dt, **CFG["bench"])
                assert _direct(ctx) == (pinned and out_dt != np.float32), (out_dt, pinned)
                assert_same(got, want)
                assert t[0] > 0 and t[1] > 0


@pytest.mark.parametrize("cfg", list(CFG))
def test_windows_layer_counts_and_k(ctx, cfg):
    rng = np.random.default_rng(42)
    h, w, n = 37, 70, 9
    for L, k, out_dt in ((1, 1, np.uint8), (4, 2, np.float16), (16, 1, np.float32), (3, 0, np.uint8), (2, 4, np.float32)):
        frames = frames_of(rng, n, h, w, np.float32)
        layers = layers_of(rng, n, L, h, w)
        got, _ = ctx.sequence_nlm_layers_temporal(frames, layers, k, hparam=H, out_dtype=out_dt, **CFG[cfg])
        assert_same(got, resident(ctx, frames, layers, k, out_dt, cfg))


def test_a_sub_range_reads_its_halo_and_two_blocks_are_the_whole_sequence(ctx):
    rng = np.random.default_rng(43)
    h, w, n, k = 40, 90, 14, 2
    frames = frames_of(rng, n, h, w, np.float32)
    layers = layers_of(rng, n, 3, h, w)
    whole, _ = ctx.sequence_nlm_layers_temporal(frames, layers, k, hparam=H, out_dtype=np.uint8, **CFG["ref"])
    assert_same(whole, resident(ctx, frames, layers, k, np.uint8, "ref"))
    sub, _ = ctx.sequence_nlm_layers_temporal(frames, layers, k, first=5, count=4, hparam=H, out_dtype=np.uint8, **CFG["ref"])
    assert_same(sub, whole[5:9])
    ups, outs = ctx.pipe_last_timeline()
    assert [u[0] for u in ups] == list(range(3, 11)) and [o[0] for o in outs] == [5, 6, 7, 8]       # the block and k halo frames on either side
    # two blocks, each given ONLY its own frames plus k halo frames (what a device of a sharded run holds)
    start, cnt = ctypes.c_int(), ctypes.c_int()
    both = []
    for g in range(2):
        assert mid.lib.mid_shard_block(n, 2, g, ctypes.byref(start), ctypes.byref(cnt)) == 0
        lo, hi = max(0, start.value - k), min(n, start.value + cnt.value + k)
        part, _ = ctx.sequence_nlm_layers_temporal(frames[lo:hi], layers[lo:hi], k, first=start.value - lo, count=cnt.value,
                                                   hparam=H, out_dtype=np.uint8, **CFG["ref"])
        both += part
    assert_same(both, whole)


def test_the_timeline_is_filled_and_each_output_uses_its_window(ctx):
    rng = np.random.default_rng(44)
    h, w, n, k = 40, 90, 6, 1
    frames = frames_of(rng, n, h, w, np.float32)
    layers = layers_of(rng, n, 2, h, w)
    got, _ = ctx.sequence_nlm_layers_temporal(frames, layers, k, hparam=H, **CFG["ref"])
    ups, outs = ctx.pipe_last_timeline()
    assert [u[0] for u in ups] == list(range(n)) and [o[0] for o in outs] == list(range(n))
    assert all(e >= s for _, s, e in ups) and all(ke > ks and de >= ds for _, ks, ke, ds, de in outs)
    # permuting the neighbours' layers changes the outputs, and to what the resident call gives for the permuted sequence
    swapped = [layers[p] for p in (1, 0, 3, 2, 5, 4)]
    got2, _ = ctx.sequence_nlm_layers_temporal(frames, swapped, k, hparam=H, **CFG["ref"])
    assert_same(got2, resident(ctx, frames, swapped, k, np.float32, "ref"))
    assert not np.array_equal(got[2], got2[2])
    got, _ = ctx.sequence_nlm_layers_temporal(frames, [[]] * n, k, hparam=H, out_dtype=np.uint8, **CFG["ref"])
    for g in got:
        assert np.array_equal(g, np.broadcast_to(np.uint8([255, 0, 255, 255]), g.shape))


def test_refusals(ctx):
    rng = np.random.default_rng(45)
    h, w, n = 24, 40, 4
    frames = frames_of(rng, n, h, w, np.float32)
    layers = layers_of(rng, n, 1, h, w)
    seq = ctx.sequence_nlm_layers_temporal
    with pytest.raises(mid.MidError):
        seq(frames, [l * 17 for l in layers], 1, hparam=H, **CFG["ref"])                       # 17 layers per frame
    with pytest.raises(mid.MidError):
        seq(frames, layers, 1, hparam=H, search=(-40, 40), patch=(-3, 3))
    for k, first, count in ((-1, 0, n), (1, -1, 2), (1, 0, 0), (1, 2, 3), (48, 0, n)):          # bad k, first, count; 2k+2 > 96
        with pytest.raises(mid.MidError):
            seq(frames, layers, k, first=first, count=count, hparam=H, **CFG["ref"])
    with pytest.raises(mid.MidError) as e:                                                     # the pointer table: a window of 11 frames x 17 pointers
        big = frames_of(rng, 4, h, w, np.float32) * 3
        seq(big, [layers[0] * 16] * 12, 5, hparam=H, **CFG["ref"])
    assert "176" in str(e.value)
    hin = [f.ctypes.data for f in frames]
    hl = [l[0].ctypes.data for l in layers]
    P = ctx.sequence_nlm_layers_temporal_pinned
    outs = [np.zeros((h, w, 4), np.float32) for _ in range(n)]
    ho = [o.ctypes.data for o in outs]
    with pytest.raises(mid.MidError):                                                          # an output is a frame of the halo
        P(hin, [ho[0], hin[3]], w, h, mid.FMT_RGBA32F, hl, 1, 1, first=1, count=2, hparam=H, **CFG["ref"])
    with pytest.raises(mid.MidError):                                                          # an output is a layer
        P(hin, [hl[0], ho[1]], w, h, mid.FMT_RGBA32F, hl, 1, 1, first=1, count=2, hparam=H, **CFG["ref"])
    with pytest.raises(mid.MidError):                                                          # an output appears twice
        P(hin, [ho[0], ho[0]], w, h, mid.FMT_RGBA32F, hl, 1, 1, first=1, count=2, hparam=H, **CFG["ref"])
    with pytest.raises(mid.MidError):                                                          # a NULL frame inside the range's halo
        P([hin[0], hin[1], hin[2], None], ho[:2], w, h, mid.FMT_RGBA32F, hl, 1, 1, first=1, count=2, hparam=H, **CFG["ref"])
    with pytest.raises(mid.MidError):                                                          # a NULL layer
        P(hin, ho[:2], w, h, mid.FMT_RGBA32F, [hl[0], None, hl[2], hl[3]], 1, 1, first=1, count=2, hparam=H, **CFG["ref"])
    with pytest.raises(mid.MidError):                                                          # a NULL output
        P(hin, [ho[0], None], w, h, mid.FMT_RGBA32F, hl, 1, 1, first=1, count=2, hparam=H, **CFG["ref"])
    # a frame outside [first-k, first+count+k) is never read: it may be NULL
    P([hin[0], hin[1], hin[2], None], ho[:1], w, h, mid.FMT_RGBA32F, hl, 1, 1, first=0, count=1, hparam=H, **CFG["ref"])
    want = ctx.nlm_layers_temporal(frames, layers, 1, 0, 1, hparam=H, **CFG["ref"])[0]
    assert np.array_equal(outs[0], want)
