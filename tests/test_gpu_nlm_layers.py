"""Layer-guided NLM on the GPU (mid_nlm_layers_accum / mid_nlm_layers): the float64 checker for every window class, the fused call
against its chain of accumulate dispatches bit for bit, the identity with plain NLM, the input formats, closed forms at 1080p
that show the guide -- not the input -- sets the weights, and the refusals."""
import ctypes

import numpy as np
import pytest

import image_denoising_filter_amd as mid
import np_nlm_layers
from conftest import rel_err

pytestmark = pytest.mark.gpu

# the window classes of test_gpu_parity.NLM_CFGS (copied: test modules are not imported)
NLM_CFGS = {"ref": dict(search=(-7, 7), patch=(-3, 3)), "bench": dict(search=(-10, 11), patch=(-3, 4)),
            "generic": dict(search=(-3, 4), patch=(-1, 2)), "rt7": dict(search=(-6, 9), patch=(-3, 4)),
            "rt5": dict(search=(-12, 13), patch=(-2, 3)), "rt4": dict(search=(-4, 5), patch=(-2, 2)),
            "rt2": dict(search=(-4, 5), patch=(-1, 1)), "rt1": dict(search=(-6, 7), patch=(0, 1)),
            "rt10": dict(search=(-3, 4), patch=(-5, 5)), "rt11": dict(search=(-5, 6), patch=(-5, 6)),
            "rt12": dict(search=(-2, 3), patch=(-6, 6)), "rt13": dict(search=(-4, 5), patch=(-6, 7)),
            "rt16": dict(search=(-2, 3), patch=(-8, 8)), "naive": dict(search=(-2, 3), patch=(-1, 3))}
TOL = 2e-5
H = 0.5


def noisy(rng, h, w, translucent=False):
    """float32 input: smooth colours + noise, alpha 1 (some 0.5 texels with `translucent`: the non-opaque form)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([0.5 + 0.4 * np.sin(xx * 0.1), 0.5 + 0.4 * np.cos(yy * 0.13), 0.3 + 0.002 * (xx + yy), np.ones_like(xx)], -1)
    img = base + np.concatenate([rng.normal(0, 0.05, (h, w, 3)), np.zeros((h, w, 1))], -1)
    img = img.astype(np.float32)
    if translucent:
        img[rng.random((h, w)) < 0.03, 3] = 0.5
    return img


def guides(rng, h, w, L):
    """RGBA8 guides close enough to each other that many weights are neither 0 nor 1 at h = 0.5."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(L):
        g = np.stack([(xx * (1 + i)) % 256, (yy * 2 + 7 * i) % 256, (xx + yy) // 2 % 256, np.full_like(xx, 255)], -1)
        g = g + rng.integers(-3, 4, (h, w, 4))
        out.append(np.clip(g, 0, 255).astype(np.uint8))
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


@pytest.mark.parametrize("cfg", list(NLM_CFGS))
@pytest.mark.parametrize("shape", [(30, 61), (37, 64)])
def test_checker_agreement(ctx, cfg, shape):
    rng = np.random.default_rng(sum(shape) + len(cfg))
    h, w = shape
    img = noisy(rng, h, w, translucent=shape[0] == 37)
    gl = guides(rng, h, w, 16)
    for L in (1, 3, 16):
        got = ctx.nlm_layers(img, gl[:L], H, **NLM_CFGS[cfg])
        want = np_nlm_layers.nlm_layers(img, gl[:L], H, **NLM_CFGS[cfg])
        assert rel_err(got, want) < TOL, (cfg, L)


@pytest.mark.parametrize("cfg", list(NLM_CFGS))
@pytest.mark.parametrize("translucent", [False, True])
def test_fused_equals_the_accumulate_chain(ctx, cfg, translucent):
    rng = np.random.default_rng(7)
    h, w = 45, 133
    img = noisy(rng, h, w, translucent)
    gl = guides(rng, h, w, 3)
    W = np.zeros((h, w, 8), np.float32)
    for g in gl:
        W = ctx.nlm_layers_accum(img, g, W, H, **NLM_CFGS[cfg])
    chain = ctx.normalize(W)
    fused = ctx.nlm_layers(img, gl, H, **NLM_CFGS[cfg])
    assert np.array_equal(bits(fused), bits(chain)), cfg


@pytest.mark.parametrize("cfg", ["ref", "naive"])
@pytest.mark.parametrize("translucent", [False, True])
def test_sixteen_layers_are_the_chain_and_the_checker(ctx, cfg, translucent):
    """The most layers one call takes (a window of one frame and 16 layer pointers in the kernel's argument block), on a frame of
    two tile rows, one of them partial, and three tile columns: the bits of 16 accumulate dispatches + normalize, and the checker."""
    rng = np.random.default_rng(16)
    h, w = 70, 130
    img = noisy(rng, h, w, translucent)
    gl = guides(rng, h, w, 16)
    assert len({g.tobytes() for g in gl}) == 16
    W = np.zeros((h, w, 8), np.float32)
    for g in gl:
        W = ctx.nlm_layers_accum(img, g, W, H, **NLM_CFGS[cfg])
    fused = ctx.nlm_layers(img, gl, H, **NLM_CFGS[cfg])
    assert np.array_equal(bits(fused), bits(ctx.normalize(W))), cfg
    assert rel_err(fused, np_nlm_layers.nlm_layers(img, gl, H, **NLM_CFGS[cfg])) < TOL, cfg


@pytest.mark.parametrize("cfg", ["ref", "bench", "generic", "naive"])
def test_input_as_its_own_guide_is_plain_nlm(ctx, cfg):
    rng = np.random.default_rng(8)
    h, w = 70, 150
    img = np.clip(noisy(rng, h, w) * 255, 0, 255).astype(np.uint8)
    got = ctx.nlm_layers(img, [img], H, **NLM_CFGS[cfg])
    want = ctx.nlm_temporal([img], k=0, hparam=H, **NLM_CFGS[cfg])[0]
    assert rel_err(got, want) < TOL


@pytest.mark.parametrize("cfg", ["ref", "bench", "naive"])
def test_half_input_is_the_widened_frame(ctx, cfg):
    rng = np.random.default_rng(9)
    h, w = 50, 90
    img = noisy(rng, h, w, translucent=True).astype(np.float16)
    gl = guides(rng, h, w, 2)
    assert np.array_equal(bits(ctx.nlm_layers(img, gl, H, **NLM_CFGS[cfg])),
                          bits(ctx.nlm_layers(img.astype(np.float32), gl, H, **NLM_CFGS[cfg])))
    u8 = np.clip(noisy(rng, h, w) * 255, 0, 255).astype(np.uint8)
    want = np_nlm_layers.nlm_layers(u8, gl, H, **NLM_CFGS[cfg])
    assert rel_err(ctx.nlm_layers(u8, gl, H, **NLM_CFGS[cfg]), want) < TOL


@pytest.mark.parametrize("out_dt", [np.uint8, np.float16])
def test_packed_outputs_are_the_packed_float_output(ctx, out_dt):
    rng = np.random.default_rng(10)
    h, w = 40, 70
    img = noisy(rng, h, w)
    gl = guides(rng, h, w, 2)
    ref = ctx.nlm_layers(img, gl, H, **NLM_CFGS["bench"])
    outs, _ = ctx.sequence_nlm_layers([img], [gl], hparam=H, out_dtype=out_dt, **NLM_CFGS["bench"])
    want = ctx.pack_u8(ref) if out_dt == np.uint8 else ctx.pack_f16(ref)
    assert np.array_equal(bits(outs[0]), bits(want))


def test_no_layers_is_magenta(ctx):
    img = noisy(np.random.default_rng(11), 33, 70)
    for cfg in ("ref", "naive"):
        out = ctx.nlm_layers(img, [], H, **NLM_CFGS[cfg])
        assert (out == np.array([1.0, 0.0, 1.0, 1.0], np.float32)).all()


def _box_sums(img, search):
    """sum of img over the search window of every pixel whose window is inside the image: [h - SW + 1, w - SW + 1, 4]."""
    SW = search[1] - search[0]
    c = np.zeros((img.shape[0] + 1, img.shape[1] + 1, 4))
    c[1:, 1:] = img.astype(np.float64).cumsum(0).cumsum(1)
    return c[SW:, SW:] - c[:-SW, SW:] - c[SW:, :-SW] + c[:-SW, :-SW]


def test_1080p_constant_guide_is_the_box_mean(ctx):
    rng = np.random.default_rng(12)
    h, w = 1080, 1920
    cfg = NLM_CFGS["bench"]
    img = rng.random((h, w, 4)).astype(np.float32)
    img[..., 3] = 1.0
    out = ctx.nlm_layers(img, [np.full((h, w, 4), 77, np.uint8)], H, **cfg)
    S = cfg["search"][1] - cfg["search"][0]
    m = 13                                   # max |s| + max |q|: every guide texel of the window is inside the image
    box = _box_sums(img, cfg["search"])      # box[y + search_lo, x + search_lo] is pixel (y, x)'s window
    want = box[m + cfg["search"][0]:h - m + cfg["search"][0], m + cfg["search"][0]:w - m + cfg["search"][0]] / (S * S + 0.001)
    assert rel_err(out[m:h - m, m:w - m], want) < TOL


def test_1080p_step_edge_guide_sets_the_weights(ctx):
    # guide 0 left of column xe, 255 from xe on (rgb): at h = 0.05 one differing texel gives exp(-1200) = 0 in fp32, so a pixel
    # whose patch lies in one region averages the input over exactly the offsets whose patch lies in that region -- the input,
    # independent noise, plays no part in the weights
    rng = np.random.default_rng(13)
    h, w, xe, hp = 1080, 1920, 960, 0.05
    cfg = NLM_CFGS["bench"]
    (slo, shi), (plo, phi) = cfg["search"], cfg["patch"]
    img = rng.random((h, w, 4)).astype(np.float32)
    img[..., 3] = 1.0
    g = np.zeros((h, w, 4), np.uint8)
    g[:, xe:, :3] = 255
    g[..., 3] = 255
    out = ctx.nlm_layers(img, [g], hp, **cfg)
    ys = slice(13, h - 13)
    colsum = img[:, :, :].astype(np.float64)
    for x in range(xe - 20, xe + 20):
        if x + phi - 1 < xe:        # patch in the left region: offsets whose patch stays left of xe
            sxs = [sx for sx in range(slo, shi) if x + sx + phi - 1 < xe]
        elif x + plo >= xe:         # patch in the right region
            sxs = [sx for sx in range(slo, shi) if x + sx + plo >= xe]
        else:
            continue
        c = np.zeros((h, 4))
        for sx in sxs:
            c += colsum[:, x + sx]
        cs = np.zeros((h + 1, 4))
        cs[1:] = c.cumsum(0)
        ywin = cs[np.arange(h)[ys] + shi] - cs[np.arange(h)[ys] + slo]
        want = ywin / (len(sxs) * (shi - slo) + 0.001)
        assert rel_err(out[ys, x], want) < TOL, x


def test_1080p_four_layers_every_pixel(ctx):
    rng = np.random.default_rng(14)
    h, w = 1080, 1920
    cfg = NLM_CFGS["ref"]
    img = noisy(rng, h, w, translucent=True)
    gl = guides(rng, h, w, 4)
    assert rel_err(ctx.nlm_layers(img, gl, H, **cfg), np_nlm_layers.nlm_layers(img, gl, H, **cfg)) < TOL


def test_refusals(ctx):
    h, w = 16, 32
    d_in, d_l, d_out, d_w = ctx.alloc(w * h * 16), ctx.alloc(w * h * 4), ctx.alloc(w * h * 16), ctx.alloc(w * h * 32)
    p = mid.NlmParams(w, h, H, -7, 7, -3, 3, mid.FMT_RGBA32F)
    tbl = (ctypes.c_void_p * 17)(*([d_l.ptr] * 17))
    L = mid.lib.mid_nlm_layers
    assert L(ctx.handle, ctypes.byref(p), d_in.ptr, tbl, 17, d_out.ptr, None) == 1           # n_layers outside 0..16
    assert L(ctx.handle, ctypes.byref(p), d_in.ptr, tbl, -1, d_out.ptr, None) == 1
    assert L(ctx.handle, ctypes.byref(p), d_in.ptr, tbl, 1, d_in.ptr, None) == 1             # out is the input
    assert L(ctx.handle, ctypes.byref(p), d_in.ptr, tbl, 1, d_l.ptr, None) == 1              # out is a layer
    ph = mid.NlmParams(w, h, H, -7, 7, -3, 3, mid.FMT_RGBA16F)
    assert L(ctx.handle, ctypes.byref(ph), d_in.ptr + 4, tbl, 1, d_out.ptr, None) == 1       # misaligned RGBA16F input
    assert mid.lib.mid_nlm_layers_accum(ctx.handle, ctypes.byref(ph), d_in.ptr + 4, d_l.ptr, d_w.ptr, None) == 1
    for bad in (mid.NlmParams(w, h, H, -40, 40, -3, 3, mid.FMT_RGBA32F),    # search wider than 64
                mid.NlmParams(w, h, H, -7, 7, -9, 9, mid.FMT_RGBA32F),      # patch wider than 16
                mid.NlmParams(w, h, H, 1, 7, -3, 3, mid.FMT_RGBA32F),       # range without 0
                mid.NlmParams(w, h, 0.0, -7, 7, -3, 3, mid.FMT_RGBA32F)):
        assert L(ctx.handle, ctypes.byref(bad), d_in.ptr, tbl, 1, d_out.ptr, None) == 1
        assert mid.lib.mid_nlm_layers_accum(ctx.handle, ctypes.byref(bad), d_in.ptr, d_l.ptr, d_w.ptr, None) == 1
    assert L(ctx.handle, ctypes.byref(p), d_in.ptr, tbl, 2, d_out.ptr, None) == 0
    ctx.sync()
