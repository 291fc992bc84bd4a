"""Layer-guided NLM over neighbouring frames on the GPU (mid_nlm_layers_pair_accum / mid_nlm_layers_temporal): the float64 checker
for every window class, window widths, layer counts and sequence lengths; the fused call against its chain of pair dispatches,
the pair dispatch with equal guides against mid_nlm_layers_accum and k = 0 against mid_nlm_layers, all bit for bit; the input and
output formats; closed forms at 1080p through the strip kernel; and the refusals."""
import ctypes

import numpy as np
import pytest

import image_denoising_filter_amd as mid
import np_nlm_layers_temporal as chk
from conftest import rel_err
from test_gpu_nlm_layers import H, NLM_CFGS, TOL, bits, guides, noisy

pytestmark = pytest.mark.gpu

MAGENTA = np.array([1.0, 0.0, 1.0, 1.0], np.float32)


def sequence(rng, h, w, n, L, translucent=False):
    """n noisy frames of one scene and, per frame, L guides that differ a little from frame to frame (many weights neither 0 nor 1)."""
    base = guides(rng, h, w, L)
    frames = [noisy(rng, h, w, translucent) for _ in range(n)]
    layers = [[np.clip(g.astype(np.int16) + rng.integers(-2, 3, g.shape), 0, 255).astype(np.uint8) for g in base] for _ in range(n)]
    return frames, layers


def chain(ctx, frames, layers, k, t, cfg, hp=H):
    """Output t as the header states it: zero W, one pair dispatch per (neighbour, layer), normalize."""
    h, w = frames[0].shape[:2]
    W = np.zeros((h, w, 8), np.float32)
    for f in range(max(0, t - k), min(len(frames) - 1, t + k) + 1):
        for l in range(len(layers[t])):
            W = ctx.nlm_layers_pair_accum(layers[t][l], layers[f][l], frames[f], W, hp, **cfg)
    return ctx.normalize(W)


@pytest.mark.parametrize("cfg", list(NLM_CFGS))
@pytest.mark.parametrize("shape", [(30, 61), (37, 64)])
def test_checker_agreement(ctx, cfg, shape):
    rng = np.random.default_rng(sum(shape) + len(cfg))
    h, w = shape
    frames, layers = sequence(rng, h, w, 5, 3, translucent=shape[0] == 37)
    cache = {}      # the sums of dispatch (t, f, l) are the same for every k, L and prefix of the sequence
    worst = 0.0
    for n in (1, 2, 5):
        for k in (1, 2):
            for L in (1, 3):
                ll = [ls[:L] for ls in layers[:n]]
                got = ctx.nlm_layers_temporal(frames[:n], ll, k, hparam=H, **NLM_CFGS[cfg])
                want = chk.nlm_layers_temporal(frames[:n], layers[:n], k, H, **NLM_CFGS[cfg], n_layers=L, cache=cache)
                for t in range(n):
                    e = rel_err(got[t], want[t])
                    worst = max(worst, e)
                    assert e < TOL, (cfg, n, k, L, t, e)
    # sub-ranges [first, first+count): the frames outside them are read only as halo
    for k, first, count in ((1, 1, 3), (2, 3, 2), (2, 0, 1)):
        got = ctx.nlm_layers_temporal(frames, layers, k, first, count, hparam=H, **NLM_CFGS[cfg])
        want = chk.nlm_layers_temporal(frames, layers, k, H, **NLM_CFGS[cfg], first=first, count=count, cache=cache)
        assert len(got) == count
        for i in range(count):
            assert rel_err(got[i], want[i]) < TOL, (cfg, k, first, i)
    print(f"{cfg} {shape}: worst rel err {worst:.2e}")


@pytest.mark.parametrize("cfg", list(NLM_CFGS))
@pytest.mark.parametrize("translucent", [False, True])
def test_fused_equals_the_chain_of_pair_dispatches(ctx, cfg, translucent):
    rng = np.random.default_rng(21)
    h, w = 45, 133
    frames, layers = sequence(rng, h, w, 4, 2, translucent)
    if translucent:
        frames[2][..., 3] = 1.0            # one opaque neighbour among translucent ones: the form is chosen per neighbour tile
    fused = ctx.nlm_layers_temporal(frames, layers, 2, hparam=H, **NLM_CFGS[cfg])
    for t in range(4):
        assert np.array_equal(bits(fused[t]), bits(chain(ctx, frames, layers, 2, t, NLM_CFGS[cfg]))), (cfg, t)


@pytest.mark.parametrize("cfg", list(NLM_CFGS))
def test_pair_accum_with_equal_guides_is_nlm_layers_accum(ctx, cfg):
    rng = np.random.default_rng(22)
    h, w = 45, 133
    for translucent in (False, True):
        img = noisy(rng, h, w, translucent)
        g = guides(rng, h, w, 1)[0]
        W = rng.random((h, w, 8), dtype=np.float32)
        a = ctx.nlm_layers_pair_accum(g, g, img, W, H, **NLM_CFGS[cfg])
        b = ctx.nlm_layers_pair_accum(g, g.copy(), img, W, H, **NLM_CFGS[cfg])       # equal texels in two buffers
        want = ctx.nlm_layers_accum(img, g, W, H, **NLM_CFGS[cfg])
        assert np.array_equal(bits(a), bits(want)) and np.array_equal(bits(b), bits(want)), (cfg, translucent)


@pytest.mark.parametrize("cfg", list(NLM_CFGS))
def test_k0_is_nlm_layers(ctx, cfg):
    rng = np.random.default_rng(23)
    h, w = 45, 133
    frames, layers = sequence(rng, h, w, 3, 3, translucent=True)
    got = ctx.nlm_layers_temporal(frames, layers, 0, hparam=H, **NLM_CFGS[cfg])
    for t in range(3):
        assert np.array_equal(bits(got[t]), bits(ctx.nlm_layers(frames[t], layers[t], H, **NLM_CFGS[cfg]))), (cfg, t)


@pytest.mark.parametrize("cfg", ["ref", "bench", "naive"])
def test_packed_inputs_are_the_widened_frames(ctx, cfg):
    rng = np.random.default_rng(24)
    h, w = 50, 90
    frames, layers = sequence(rng, h, w, 3, 2, translucent=True)
    half = [f.astype(np.float16) for f in frames]
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(
        ctx.nlm_layers_temporal(half, layers, 1, hparam=H, **NLM_CFGS[cfg]),
        ctx.nlm_layers_temporal([f.astype(np.float32) for f in half], layers, 1, hparam=H, **NLM_CFGS[cfg])))
    u8 = [np.clip(noisy(rng, h, w) * 255, 0, 255).astype(np.uint8) for _ in range(3)]
    wide = [ctx.unpack_u8(f) for f in u8]
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(
        ctx.nlm_layers_temporal(u8, layers, 1, hparam=H, **NLM_CFGS[cfg]),
        ctx.nlm_layers_temporal(wide, layers, 1, hparam=H, **NLM_CFGS[cfg])))


@pytest.mark.parametrize("cfg", ["ref", "bench", "naive"])
@pytest.mark.parametrize("out_dt", [np.uint8, np.float16])
def test_packed_outputs_are_the_packed_float_output(ctx, cfg, out_dt):
    rng = np.random.default_rng(25)
    h, w = 40, 70
    frames, layers = sequence(rng, h, w, 3, 2)
    ref = ctx.nlm_layers_temporal(frames, layers, 1, hparam=H, **NLM_CFGS[cfg])
    got = ctx.nlm_layers_temporal(frames, layers, 1, hparam=H, out_dtype=out_dt, **NLM_CFGS[cfg])
    for r, g in zip(ref, got):
        assert np.array_equal(bits(g), bits(ctx.pack_u8(r) if out_dt == np.uint8 else ctx.pack_f16(r)))


def test_no_layers_is_magenta(ctx):
    frames = [noisy(np.random.default_rng(26), 33, 70) for _ in range(3)]
    for cfg in ("ref", "naive"):
        for out in ctx.nlm_layers_temporal(frames, [[], [], []], 1, hparam=H, **NLM_CFGS[cfg]):
            assert (out == MAGENTA).all()


def _zero_padded_box(img, search):
    """out[y, x] = sum of img over the search window of (y, x), texels outside the image 0: [h, w, 4] float64."""
    slo, shi = search
    h, w = img.shape[:2]
    P = max(-slo, shi)
    c = np.zeros((h + 2 * P + 1, w + 2 * P + 1, 4))
    c[1:, 1:] = np.pad(img.astype(np.float64), ((P, P), (P, P), (0, 0))).cumsum(0).cumsum(1)
    y0, x0 = P + slo, P + slo
    S = shi - slo
    return c[y0 + S:y0 + S + h, x0 + S:x0 + S + w] - c[y0:y0 + h, x0 + S:x0 + S + w] - c[y0 + S:y0 + S + h, x0:x0 + w] + c[y0:y0 + h, x0:x0 + w]


def _flat(h, w, byte):
    g = np.full((h, w, 4), byte, np.uint8)
    g[..., 3] = 255
    return g


@pytest.mark.parametrize("cfg", ["ref", "bench"])
def test_1080p_constant_layers_are_the_box_mean_over_the_window(ctx, cfg):
    # every weight is 1: out = sum_f box_f / (m (S^2 + 0.001)), L cancels.  A non-zero constant holds where search and patch windows
    # stay inside the image (out-of-image guide texels are 0 and mismatch it); the constant 0 holds at every pixel.
    rng = np.random.default_rng(27)
    h, w, n, k = 1080, 1920, 3, 1
    (slo, shi), (plo, phi) = NLM_CFGS[cfg]["search"], NLM_CFGS[cfg]["patch"]
    S = shi - slo
    m = max(-slo, shi - 1) + max(-plo, phi - 1)
    frames = []
    for _ in range(n):
        f = rng.random((h, w, 4)).astype(np.float32)
        f[..., 3] = 1.0
        frames.append(f)
    boxes = [_zero_padded_box(f, (slo, shi)) for f in frames]
    for byte, L, inner in ((77, 2, (slice(m, h - m), slice(m, w - m))), (0, 1, (slice(None), slice(None)))):
        layers = [[_flat(h, w, byte)] * L for _ in range(n)]
        got = ctx.nlm_layers_temporal(frames, layers, k, hparam=H, **NLM_CFGS[cfg])
        for t in range(n):
            win = range(max(0, t - k), min(n - 1, t + k) + 1)
            want = sum(boxes[f] for f in win) / (len(win) * (S * S + 0.001))
            e = rel_err(got[t][inner], want[inner])
            print(f"{cfg} constant {byte} output {t}: {e:.2e}")
            assert e < TOL, (cfg, byte, t, e)


@pytest.mark.parametrize("cfg", ["ref", "bench"])
def test_1080p_a_mismatching_neighbour_is_switched_off(ctx, cfg):
    # frames 0, 1: layers byte 0; frame 2: layers byte 255; h = 0.05: one mismatching texel gives exp(-1200) = 0 in fp32.  Interior
    # pixels of output 1 (window 0, 1, 2): frames 0 and 1 with every weight 1, frame 2 adds only its 0.001 per dispatch.
    rng = np.random.default_rng(28)
    h, w, n, k, hp, L = 1080, 1920, 3, 1, 0.05, 2
    (slo, shi), (plo, phi) = NLM_CFGS[cfg]["search"], NLM_CFGS[cfg]["patch"]
    S = shi - slo
    m = max(-slo, shi - 1) + max(-plo, phi - 1)
    frames = []
    for _ in range(n):
        f = rng.random((h, w, 4)).astype(np.float32)
        f[..., 3] = 1.0
        frames.append(f)
    layers = [[_flat(h, w, 0)] * L, [_flat(h, w, 0)] * L, [_flat(h, w, 255)] * L]
    got = ctx.nlm_layers_temporal(frames, layers, k, hparam=hp, **NLM_CFGS[cfg])
    boxes = [_zero_padded_box(f, (slo, shi)) for f in frames]
    inner = (slice(m, h - m), slice(m, w - m))
    want0 = (boxes[0] + boxes[1]) / (2 * (S * S + 0.001))                    # output 0: window 0, 1 -- every pixel
    want1 = (boxes[0] + boxes[1]) / (2 * (S * S + 0.001) + 0.001)            # output 1: frame 2 switched off
    want2 = boxes[2] / ((S * S + 0.001) + 0.001)                             # output 2: its own frame only, frame 1 switched off
    e0, e1, e2 = rel_err(got[0], want0), rel_err(got[1][inner], want1[inner]), rel_err(got[2][inner], want2[inner])
    print(f"{cfg} switched-off neighbour: {e0:.2e} {e1:.2e} {e2:.2e}")
    assert e0 < TOL and e1 < TOL and e2 < TOL


def test_1080p_noisy_sequence_every_pixel(ctx):
    # output 1 of 3 frames, k = 1: the whole window, two layers, translucent texels, every pixel against the checker
    rng = np.random.default_rng(29)
    h, w = 1080, 1920
    frames, layers = sequence(rng, h, w, 3, 2, translucent=True)
    got = ctx.nlm_layers_temporal(frames, layers, 1, 1, 1, hparam=H, **NLM_CFGS["ref"])[0]
    want = chk.nlm_layers_temporal(frames, layers, 1, H, **NLM_CFGS["ref"], first=1, count=1)[0]
    e = rel_err(got, want)
    print(f"1080p noisy 3 frames x 2 layers, output 1: {e:.2e}")
    assert e < TOL


def test_refusals(ctx):
    h, w, n, L = 16, 32, 3, 2
    d_fr = [ctx.alloc(w * h * 16) for _ in range(n)]
    d_l = [ctx.alloc(w * h * 4) for _ in range(n * L)]
    d_out = [ctx.alloc(w * h * 16) for _ in range(n)]
    d_w = ctx.alloc(w * h * 32)
    p = ctypes.byref(mid.NlmParams(w, h, H, -7, 7, -3, 3, mid.FMT_RGBA32F))
    T, P = mid.lib.mid_nlm_layers_temporal, mid.lib.mid_nlm_layers_pair_accum
    fr = (ctypes.c_void_p * n)(*[d.ptr for d in d_fr])
    ly = (ctypes.c_void_p * (n * L))(*[d.ptr for d in d_l])
    out = (ctypes.c_void_p * n)(*[d.ptr for d in d_out])

    def call(frames=fr, layers=ly, n_layers=L, n_frames=n, k=1, first=0, count=n, outs=out, fmt=mid.FMT_RGBA32F, prm=p):
        return T(ctx.handle, prm, frames, layers, n_layers, n_frames, k, first, count, outs, fmt, None)

    assert call() == 0
    assert call(frames=None) == 1 and call(outs=None) == 1 and call(layers=None) == 1 and call(prm=None) == 1     # NULL tables
    assert call(layers=None, n_layers=0) == 0                                                                      # (no layers: none needed)
    for tbl, size, key in ((fr, n, "frames"), (ly, n * L, "layers"), (out, n, "outs")):                            # a NULL entry
        bad = (ctypes.c_void_p * size)(*tbl)
        bad[1] = None
        assert call(**{key: bad}) == 1, key
    assert call(n_layers=17, layers=(ctypes.c_void_p * 51)(*([d_l[0].ptr] * 51))) == 1 and call(n_layers=-1) == 1
    assert call(outs=(ctypes.c_void_p * n)(d_out[0].ptr, d_fr[2].ptr, d_out[2].ptr)) == 1                          # out is a frame
    assert b"out[1]" in mid.lib.mid_last_error()
    assert call(outs=(ctypes.c_void_p * n)(d_out[0].ptr, d_out[1].ptr, d_l[3].ptr)) == 1                           # out is a layer
    assert call(outs=(ctypes.c_void_p * n)(d_out[0].ptr, d_out[1].ptr, d_out[0].ptr)) == 1                         # out twice
    assert call(k=-1) == 1 and call(first=-1) == 1 and call(count=0) == 1 and call(first=1, count=n) == 1 and call(n_frames=0) == 1
    assert call(fmt=7) == 1
    # the pointer table of one launch: min(2k+1, n_frames) * (n_layers + 1) <= 176
    assert mid.lib.mid_version() and 11 * 17 > 176 >= 10 * 17
    big_n = 11
    fr_b = (ctypes.c_void_p * big_n)(*([d_fr[0].ptr] * big_n))
    ly_b = (ctypes.c_void_p * (big_n * 16))(*([d_l[0].ptr] * (big_n * 16)))
    assert call(frames=fr_b, layers=ly_b, n_layers=16, n_frames=big_n, k=5, first=5, count=1) == 1
    assert b"176" in mid.lib.mid_last_error()
    assert call(frames=fr_b, layers=ly_b, n_layers=15, n_frames=big_n, k=5, first=5, count=1) == 0                 # 11 * 16 = 176 fits
    ph = ctypes.byref(mid.NlmParams(w, h, H, -7, 7, -3, 3, mid.FMT_RGBA16F))
    assert call(prm=ph, frames=(ctypes.c_void_p * n)(d_fr[0].ptr, d_fr[1].ptr + 4, d_fr[2].ptr)) == 1              # misaligned RGBA16F
    assert P(ctx.handle, p, d_l[0].ptr, d_l[1].ptr, d_fr[0].ptr, d_w.ptr, None) == 0
    assert P(ctx.handle, p, None, d_l[1].ptr, d_fr[0].ptr, d_w.ptr, None) == 1
    assert P(ctx.handle, p, d_l[0].ptr, None, d_fr[0].ptr, d_w.ptr, None) == 1
    assert P(ctx.handle, p, d_l[0].ptr, d_l[1].ptr, None, d_w.ptr, None) == 1
    assert P(ctx.handle, p, d_l[0].ptr, d_l[1].ptr, d_fr[0].ptr, None, None) == 1
    assert P(ctx.handle, ph, d_l[0].ptr, d_l[1].ptr, d_fr[0].ptr + 4, d_w.ptr, None) == 1
    for bad in (mid.NlmParams(w, h, H, -40, 40, -3, 3, mid.FMT_RGBA32F), mid.NlmParams(w, h, H, -7, 7, -9, 9, mid.FMT_RGBA32F),
                mid.NlmParams(w, h, H, 1, 7, -3, 3, mid.FMT_RGBA32F), mid.NlmParams(w, h, 0.0, -7, 7, -3, 3, mid.FMT_RGBA32F)):
        assert call(prm=ctypes.byref(bad)) == 1
        assert P(ctx.handle, ctypes.byref(bad), d_l[0].ptr, d_l[1].ptr, d_fr[0].ptr, d_w.ptr, None) == 1
    ctx.sync()
