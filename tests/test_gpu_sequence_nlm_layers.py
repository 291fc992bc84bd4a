"""GPU suite: layer-guided NLM over a whole animation (mid_sequence_nlm_layers) -- output i has the bits of
ctx.nlm_layers(frame i, its own layers), packed by the kernel's epilogue for RGBA8 / RGBA16F outputs, with page-locked outputs
(stored by the kernel) and pageable ones (downloaded), with and without overlap, and for a frame block given as a sub-array."""
import numpy as np
import pytest

import image_denoising_filter_amd as mid

pytestmark = pytest.mark.gpu

H = 0.5
CFG = {"ref": dict(search=(-7, 7), patch=(-3, 3)), "bench": dict(search=(-10, 11), patch=(-3, 4)),
       "naive": dict(search=(-2, 3), patch=(-1, 3))}
OUT = (np.float32, np.uint8, np.float16)


def frames_of(rng, n, h, w, dt):
    out = []
    for _ in range(n):
        f = np.concatenate([rng.random((h, w, 3)) * 0.3 + 0.3, np.ones((h, w, 1))], -1).astype(np.float32)
        if rng.random() < 0.5:
            f[rng.random((h, w)) < 0.02, 3] = 0.5
        out.append(np.clip(f * 255, 0, 255).astype(np.uint8) if dt == np.uint8 else f.astype(dt))
    return out


def layers_of(rng, n, L, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 3 % 256, yy * 5 % 256, (xx + yy) % 256, np.full_like(xx, 255)], -1)
    return [[np.clip(base + rng.integers(-4, 5, (h, w, 4)), 0, 255).astype(np.uint8) for _ in range(L)] for _ in range(n)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def want(ctx, frames, layers, out_dt, cfg):
    out = []
    for f, ls in zip(frames, layers):
        r = ctx.nlm_layers(f, ls, H, **CFG[cfg])
        out.append(ctx.pack_u8(r) if out_dt == np.uint8 else ctx.pack_f16(r) if out_dt == np.float16 else r)
    return out


def assert_same(got, wanted):
    assert len(got) == len(wanted)
    for i, (g, w) in enumerate(zip(got, wanted)):
        assert g.dtype == w.dtype and g.shape == w.shape, i
        assert np.array_equal(bits(g), bits(w)), f"output {i} differs"


def _direct(ctx):
    _, outs = ctx.pipe_last_timeline()
    return all(ds == ke and de == ke for _, _, ke, ds, de in outs)


@pytest.mark.parametrize("in_dt", [np.float32, np.uint8, np.float16])
def test_sixteen_frames_every_output_format_and_host_memory(ctx, in_dt):
    rng = np.random.default_rng(31)
    h, w, n = 48, 100, 16
    frames = frames_of(rng, n, h, w, in_dt)
    layers = layers_of(rng, n, 2, h, w)
    for out_dt in OUT:
        wl = want(ctx, frames, layers, out_dt, "bench")
        for pinned_out in (True, False):
            for overlap in (True, False):
                got, _ = ctx.sequence_nlm_layers(frames, layers, overlap=overlap, hparam=H, pinned=pinned_out,
                                                 pinned_out=pinned_out, out_dtype=out_dt, **CFG["bench"])
                assert _direct(ctx) == (pinned_out and out_dt != np.float32), (out_dt, pinned_out)
                assert_same(got, wl)


@pytest.mark.parametrize("cfg", list(CFG))
def test_layer_counts_and_windows(ctx, cfg):
    rng = np.random.default_rng(32)
    h, w, n = 37, 70, 16
    for L, out_dt in ((1, np.uint8), (4, np.float16), (16, np.float32)):
        frames = frames_of(rng, n, h, w, np.float32)
        layers = layers_of(rng, n, L, h, w)
        got, _ = ctx.sequence_nlm_layers(frames, layers, hparam=H, out_dtype=out_dt, **CFG[cfg])
        assert_same(got, want(ctx, frames, layers, out_dt, cfg))


def test_a_frame_block_is_a_sub_array(ctx):
    rng = np.random.default_rng(33)
    h, w, n = 40, 90, 18
    frames = frames_of(rng, n, h, w, np.float32)
    layers = layers_of(rng, n, 3, h, w)
    whole, _ = ctx.sequence_nlm_layers(frames, layers, hparam=H, out_dtype=np.uint8, **CFG["ref"])
    block, _ = ctx.sequence_nlm_layers(frames[5:12], layers[5:12], hparam=H, out_dtype=np.uint8, **CFG["ref"])
    assert_same(block, whole[5:12])
    assert_same(whole, want(ctx, frames, layers, np.uint8, "ref"))


def test_each_output_uses_its_own_layers_and_no_layers_is_magenta(ctx):
    rng = np.random.default_rng(34)
    h, w, n = 40, 90, 4
    frames = frames_of(rng, n, h, w, np.float32)
    layers = layers_of(rng, n, 2, h, w)
    swapped = [layers[p] for p in (1, 0, 3, 2)]
    got, _ = ctx.sequence_nlm_layers(frames, swapped, hparam=H, **CFG["ref"])
    assert_same(got, want(ctx, frames, swapped, np.float32, "ref"))
    got, _ = ctx.sequence_nlm_layers(frames, [[]] * n, hparam=H, out_dtype=np.uint8, **CFG["ref"])
    for g in got:
        assert np.array_equal(g, np.broadcast_to(np.uint8([255, 0, 255, 255]), g.shape))
    ctx.pipe_last_timeline()


def test_refusals(ctx):
    rng = np.random.default_rng(35)
    h, w = 24, 40
    frames = frames_of(rng, 2, h, w, np.float32)
    layers = layers_of(rng, 2, 1, h, w)
    with pytest.raises(mid.MidError):
        ctx.sequence_nlm_layers(frames, [l * 17 for l in layers], hparam=H, **CFG["ref"])       # 17 layers per frame
    with pytest.raises(mid.MidError):
        ctx.sequence_nlm_layers(frames, layers, hparam=H, search=(-40, 40), patch=(-3, 3))
    hin = [f.ctypes.data for f in frames]
    hl = [l[0].ctypes.data for l in layers]
    with pytest.raises(mid.MidError):                                                          # an output is an input frame
        ctx.sequence_nlm_layers_pinned(hin, [hin[1], hin[0]], w, h, mid.FMT_RGBA32F, hl, 1, hparam=H, **CFG["ref"])
    outs = [np.zeros((h, w, 4), np.uint8) for _ in range(2)]
    with pytest.raises(mid.MidError):                                                          # an output is a layer
        ctx.sequence_nlm_layers_pinned(hin, [hl[0], outs[1].ctypes.data], w, h, mid.FMT_RGBA32F, hl, 1, hparam=H,
                                       out_dtype=np.uint8, **CFG["ref"])
