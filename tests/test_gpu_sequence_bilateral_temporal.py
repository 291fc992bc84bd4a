"""GPU suite: the bilateral over neighbouring frames through the frame pipeline (mid_sequence_bilateral_temporal) -- every output
has the bits of ctx.bilateral_temporal of the resident sequence, plain and layered, for the three input and the three output
formats, page-locked (packed outputs stored by the kernel) and pageable, with and without overlap; a block is the same outputs;
the refusals queue nothing."""
import ctypes

import numpy as np
import pytest

import image_denoising_filter_amd as mid
from test_gpu_bilateral_temporal import bits, layers_of, sig

pytestmark = pytest.mark.gpu

H, W, N, R = 45, 133, 6, 8
OUT = (np.float32, np.uint8, np.float16)


def frames_of(rng, n, h, w, dt):
    out = []
    for _ in range(n):
        f = np.concatenate([rng.random((h, w, 3)) * 0.3 + 0.3, np.ones((h, w, 1))], -1).astype(np.float32)
        if rng.random() < 0.5:
            f[rng.random((h, w)) < 0.02, 3] = 0.5
        out.append(np.clip(f * 255, 0, 255).astype(np.uint8) if dt == np.uint8 else f.astype(dt))
    return out


def assert_same(got, wanted):
    assert len(got) == len(wanted)
    for i, (g, w) in enumerate(zip(got, wanted)):
        assert g.dtype == w.dtype and g.shape == w.shape, i
        assert np.array_equal(bits(g), bits(w)), f"output {i} differs"


def _direct(ctx):
    _, outs = ctx.pipe_last_timeline()
    return all(ds == ke and de == ke for _, _, ke, ds, de in outs)


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("in_dt", [np.float32, np.uint8, np.float16])
@pytest.mark.parametrize("k", [1, 2])
def test_every_output_is_the_resident_calls(ctx, in_dt, layered, k):
    rng = np.random.default_rng(71)
    frames = frames_of(rng, N, H, W, in_dt)
    layers = layers_of(rng, N, 2, H, W) if layered else None
    for out_dt in OUT:
        want = ctx.bilateral_temporal(frames, k, radius=R, layers=layers, out_dtype=out_dt, **sig(R))
        for pinned in (True, False):
            for overlap in (True, False):
                got, t = ctx.sequence_bilateral_temporal(frames, k, overlap=overlap, radius=R, layers=layers, pinned=pinned,
                                                         pinned_out=pinned, out_dtype=out_dt, **sig(R))
                # packed outputs inside one page-locked allocation are stored by the kernel: an empty download interval
                assert _direct(ctx) == (pinned and out_dt != np.float32), (out_dt, pinned)
                assert_same(got, want)
                assert t[0] > 0 and t[1] > 0


@pytest.mark.parametrize("layered", [False, True])
def test_a_block_is_the_same_outputs(ctx, layered):
    rng = np.random.default_rng(72)
    k = 2
    frames = frames_of(rng, N, H, W, np.float32)
    layers = layers_of(rng, N, 3, H, W) if layered else None
    whole, _ = ctx.sequence_bilateral_temporal(frames, k, radius=R, layers=layers, out_dtype=np.uint8, **sig(R))
    ups, outs = ctx.pipe_last_timeline()
    assert [u[0] for u in ups] == list(range(N)) and [o[0] for o in outs] == list(range(N))
    assert all(e >= s for _, s, e in ups) and all(ke > ks and de >= ds for _, ks, ke, ds, de in outs)
    sub, _ = ctx.sequence_bilateral_temporal(frames, 1, first=3, count=2, radius=R, layers=layers, out_dtype=np.uint8, **sig(R))
    ups, outs = ctx.pipe_last_timeline()
    assert [u[0] for u in ups] == [2, 3, 4, 5] and [o[0] for o in outs] == [3, 4]       # the block and k halo frames on either side
    assert_same(sub, ctx.bilateral_temporal(frames, 1, 3, 2, radius=R, layers=layers, out_dtype=np.uint8, **sig(R)))
    both = []
    start, cnt = ctypes.c_int(), ctypes.c_int()
    for rank in range(2):
        assert mid.lib.mid_shard_block(N, 2, rank, ctypes.byref(start), ctypes.byref(cnt)) == 0
        part, _ = ctx.sequence_bilateral_temporal(frames, k, first=start.value, count=cnt.value, radius=R, layers=layers,
                                                  out_dtype=np.uint8, **sig(R))
        both += part
    assert_same(both, whole)


def test_no_layers_is_magenta(ctx):
    frames = frames_of(np.random.default_rng(73), 3, 24, 40, np.float32)
    got, _ = ctx.sequence_bilateral_temporal(frames, 1, radius=4, layers=[[]] * 3, out_dtype=np.uint8)
    for g in got:
        assert np.array_equal(g, np.broadcast_to(np.uint8([255, 0, 255, 255]), g.shape))


def test_refusals_queue_no_work(ctx):
    rng = np.random.default_rng(74)
    h, w, n = 24, 40, 4
    frames = frames_of(rng, n, h, w, np.float32)
    layers = layers_of(rng, n, 1, h, w)
    seq = ctx.sequence_bilateral_temporal
    with pytest.raises(mid.MidError):
        seq(frames, 1, radius=4, layers=[l * 17 for l in layers])                              # 17 layers per frame
    with pytest.raises(mid.MidError):
        seq(frames, 1, radius=25)
    for k, first, count in ((-1, 0, n), (1, -1, 2), (1, 0, 0), (1, 2, 3), (48, 0, n)):          # bad k, first, count; 2k+2 > 96
        with pytest.raises(mid.MidError):
            seq(frames, k, first=first, count=count, radius=4, layers=layers)
    with pytest.raises(mid.MidError) as e:                                                     # the pointer table: a window of 11 frames x 17 pointers
        seq(frames * 3, 5, radius=4, layers=[layers[0] * 16] * 12)
    assert "176" in str(e.value)
    hin = [f.ctypes.data for f in frames]
    hl = [l[0].ctypes.data for l in layers]
    outs = [np.full((h, w, 4), 7.0, np.float32) for _ in range(n)]
    ho = [o.ctypes.data for o in outs]
    lib, f32 = mid.lib, mid.FMT_RGBA32F
    t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)

    def raw(p, hin_=hin, hl_=hl, L=1, k=1, first=1, count=2, out=None, out_fmt=f32):
        out = ho[:2] if out is None else out
        return lib.mid_sequence_bilateral_temporal(ctx.handle, ctypes.byref(p), (ctypes.c_void_p * n)(*hin_), n,
                                                   None if hl_ is None else (ctypes.c_void_p * n)(*hl_), L, k, first, count,
                                                   (ctypes.c_void_p * len(out))(*out), out_fmt, 1, t)

    seq(frames, 1, radius=4, layers=layers)
    before = ctx.pipe_last_timeline()
    ok = mid.BilateralParams(w, h, 2.0, 0.2, 4, mid.LAYOUT_TEXTURE, f32)
    lin = mid.BilateralParams(w, h, 2.0, 0.2, 4, mid.LAYOUT_LINEAR, f32)
    assert raw(lin) == 1 and raw(lin, hl_=None, L=0) == 1                                      # no temporal form of the linear layout
    assert raw(ok, hl_=None, L=1) == 1                                                         # the plain form takes n_layers == 0
    assert raw(ok, out_fmt=9) == 1
    assert raw(ok, out=[ho[0], hin[3]]) == 1                                                   # an output is a frame of the halo
    assert raw(ok, out=[hl[0], ho[1]]) == 1                                                    # an output is a layer
    assert raw(ok, out=[ho[0], ho[0]]) == 1                                                    # an output appears twice
    assert raw(ok, hin_=[hin[0], hin[1], hin[2], None]) == 1                                   # a NULL frame inside the range's halo
    assert raw(ok, hl_=[hl[0], None, hl[2], hl[3]]) == 1                                       # a NULL layer
    assert raw(ok, out=[ho[0], None]) == 1                                                     # a NULL output
    d_in, d_out = ctx.upload(frames[0]), ctx.alloc(h * w * 16)
    with ctx.record() as rec:                                       # a recording with one launch in it, then the refused call
        ctx.bilateral_dev(d_in.ptr, d_out.ptr, w, h, 4, 2.0, 0.2, mid.LAYOUT_TEXTURE, f32)
        rc = raw(ok)
    assert rec.info()[0] == 1
    rec.close()
    assert rc == 1 and b"recording" in lib.mid_last_error()
    assert all((o == 7.0).all() for o in outs) and list(t) == [-1.0, -1.0, -1.0]
    assert ctx.pipe_last_timeline() == before                       # no refused call queued anything
    # a frame outside [first-k, first+count+k) is never read: it may be NULL
    assert raw(ok, hin_=[hin[0], hin[1], hin[2], None], first=0, count=1, out=ho[:1]) == 0, lib.mid_last_error()
    assert np.array_equal(outs[0], ctx.bilateral_temporal(frames, 1, 0, 1, radius=4, layers=layers)[0])
