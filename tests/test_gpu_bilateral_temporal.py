"""GPU suite: the bilateral over neighbouring frames (mid_bilateral_pair_accum, mid_bilateral_layers_pair_accum,
mid_bilateral_temporal) against its float64 checker (np_bilateral_temporal.py), against its own chain of pair dispatches and
against the single-frame kernels, bit for bit where the header says so, in every kernel class: radii 4, 8 and 20 (tuned tiles),
5 (run-time radius), 18 with layers (per pixel).  Frames of 30x61, 37x64 and 45x133: a partial tile, an exact tile width with a
ragged last row of waves, seams in both directions (tiles are 64 x 16 rows, 64 x 8 at r = 20)."""
import ctypes

import numpy as np
import pytest

import image_denoising_filter_amd as mid
import np_bilateral_temporal as chk
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5                                         # the project's bilateral tolerance (test_gpu_bilateral_fullframe.py)
SHAPES = [(30, 61), (37, 64), (45, 133)]
PLAIN_R, LAYER_R = (4, 8, 5, 20), (4, 8, 5, 20, 18)
CLASSES = [(r, False) for r in PLAIN_R] + [(r, True) for r in LAYER_R]
SC = 0.1


def sig(r):
    return dict(sigma_s=max(2.0, r / 2.5), sigma_c=SC)


def frames_of(rng, n, h, w, translucent=()):
    """n noisy float32 frames of one scene; frames listed in `translucent` get some alpha != 1 texels."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([0.5 + 0.3 * np.sin(xx * 0.21), 0.5 + 0.3 * np.cos(yy * 0.17), (xx + yy) / (h + w)], -1)
    out = []
    for i in range(n):
        f = np.concatenate([base + rng.normal(0, 0.04, (h, w, 3)), np.ones((h, w, 1))], -1).astype(np.float32)
        if i in translucent:
            f[rng.random((h, w)) < 0.05, 3] = 0.5
        out.append(f)
    return out


def layers_of(rng, n, L, h, w):
    """Guides that differ by a few codes from frame to frame, on ramps of a few codes per pixel: at colorSigma 0.1 most range
    weights are neither 0 nor 1."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = [np.stack([(xx * 5 + 40 * l) % 256, (yy * 7) % 256, (xx * 2 + yy * 3) % 256, np.full_like(xx, 255)], -1) for l in range(L)]
    return [[np.clip(b + rng.integers(-3, 4, (h, w, 4)), 0, 255).astype(np.uint8) for b in base] for _ in range(n)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def chain(ctx, frames, layers, k, r, t):
    """Output t as the header spells it: zero W, the pair dispatches in order, normalize."""
    n = len(frames)
    h, w = frames[0].shape[:2]
    W = np.zeros((h, w, 8), np.float32)
    for f in chk.window(n, t, k):
        if layers is None:
            W = ctx.bilateral_pair_accum(frames[t], frames[f], W, r, **sig(r))
        else:
            for lt, lf in zip(layers[t], layers[f]):
                W = ctx.bilateral_layers_pair_accum(lt, lf, frames[f], W, r, **sig(r))
    return ctx.normalize(W)


# ---- against the float64 checker ---------------------------------------------------------------------------------------------
# every n in {1, 2, 5}, k in {1, 2}, L in {1, 3} and every shape occurs; every output of each sequence is compared
CONFIGS = [((30, 61), 1, 1, 1), ((37, 64), 2, 2, 3), ((45, 133), 5, 1, 3), ((45, 133), 5, 2, 1)]


@pytest.mark.parametrize("r,layered", CLASSES)
def test_every_output_matches_the_checker(ctx, r, layered):
    rng = np.random.default_rng(100 + r)
    worst = 0.0
    for (h, w), n, k, L in CONFIGS:
        frames = frames_of(rng, n, h, w)
        layers = layers_of(rng, n, L, h, w) if layered else None
        got = ctx.bilateral_temporal(frames, k, radius=r, layers=layers, **sig(r))
        want = chk.bilateral_temporal(frames, k, r, layers=layers, **sig(r))
        assert len(got) == n
        errs = [rel_err(g, x) for g, x in zip(got, want)]
        print(f"r={r} layered={layered} {h}x{w} n={n} k={k} L={L}: worst rel err {max(errs):.3e}")
        worst = max(worst, max(errs))
        assert max(errs) < TOL, (h, w, n, k, L, errs)
    print(f"r={r} layered={layered}: worst rel err over all configurations {worst:.3e}")


@pytest.mark.parametrize("layered", [False, True])
@pytest.mark.parametrize("k,first,count", [(1, 1, 3), (2, 3, 2), (2, 0, 1)])
def test_sub_ranges_are_the_same_outputs(ctx, layered, k, first, count):
    rng = np.random.default_rng(7)
    h, w, n, r = 45, 133, 5, 8
    frames = frames_of(rng, n, h, w)
    layers = layers_of(rng, n, 3, h, w) if layered else None
    sub = ctx.bilateral_temporal(frames, k, first, count, radius=r, layers=layers, **sig(r))
    want = chk.bilateral_temporal(frames, k, r, layers=layers, first=first, count=count, **sig(r))
    whole = ctx.bilateral_temporal(frames, k, radius=r, layers=layers, **sig(r))
    assert len(sub) == count
    for i in range(count):
        e = rel_err(sub[i], want[i])
        print(f"k={k} output {first + i}: rel err {e:.3e}")
        assert e < TOL
        assert same(sub[i], whole[first + i])


# ---- fused == chain, bit for bit -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,layered", CLASSES)
@pytest.mark.parametrize("translucent", [(), (0, 2)], ids=["opaque", "translucent-one-opaque-neighbour"])
def test_fused_has_the_bits_of_its_chain(ctx, r, layered, translucent):
    rng = np.random.default_rng(200 + r)
    h, w, n, k = 45, 133, 3, 1
    frames = frames_of(rng, n, h, w, translucent)
    layers = layers_of(rng, n, 2, h, w) if layered else None
    got = ctx.bilateral_temporal(frames, k, radius=r, layers=layers, **sig(r))
    for t in range(n):
        assert same(got[t], chain(ctx, frames, layers, k, r, t)), t


# ---- equal guides and k = 0 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", LAYER_R)
def test_pair_with_equal_guides_is_bilateral_layers_accum(ctx, r):
    rng = np.random.default_rng(300 + r)
    h, w = 37, 64
    img = frames_of(rng, 1, h, w, (0,))[0]
    lyr = layers_of(rng, 1, 1, h, w)[0][0]
    W = rng.random((h, w, 8), dtype=np.float32)
    want = ctx.bilateral_layers_accum(img, lyr, W, r, **sig(r))
    assert not np.array_equal(want, W)
    assert same(ctx.bilateral_layers_pair_accum(lyr, lyr, img, W, r, **sig(r)), want)            # the same buffer
    assert same(ctx.bilateral_layers_pair_accum(lyr.copy(), lyr, img, W, r, **sig(r)), want)     # equal texels in two buffers


@pytest.mark.parametrize("r,layered", CLASSES)
def test_k0_is_the_single_frame_filter(ctx, r, layered):
    rng = np.random.default_rng(400 + r)
    for h, w in SHAPES:
        frames = frames_of(rng, 2, h, w, (1,))
        layers = layers_of(rng, 2, 3, h, w) if layered else None
        got = ctx.bilateral_temporal(frames, 0, radius=r, layers=layers, **sig(r))
        for t in range(2):
            want = ctx.bilateral_layers(frames[t], layers[t], r, **sig(r)) if layered else ctx.bilateral(frames[t], r, **sig(r))
            assert same(got[t], want), (h, w, t)


@pytest.mark.parametrize("r", LAYER_R)
def test_no_layers_is_magenta(ctx, r):
    frames = frames_of(np.random.default_rng(5), 3, 30, 61)
    for out in ctx.bilateral_temporal(frames, 1, radius=r, layers=[[], [], []], **sig(r)):
        assert np.array_equal(out, np.broadcast_to(np.float32([1, 0, 1, 1]), out.shape))
    assert np.array_equal(ctx.bilateral_layers(frames[0], [], r, **sig(r))[0, 0], np.float32([1, 0, 1, 1]))


# ---- formats -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,layered", [(8, False), (8, True), (5, False), (5, True), (18, True)])
def test_input_and_output_formats(ctx, r, layered):
    rng = np.random.default_rng(500 + r)
    h, w, n, k = 37, 64, 3, 1
    f32 = frames_of(rng, n, h, w)
    layers = layers_of(rng, n, 2, h, w) if layered else None
    for packed in ([f.astype(np.float16) for f in f32], [np.clip(f * 255, 0, 255).astype(np.uint8) for f in f32]):
        wide = [chk.decode(f) for f in packed]             # exact widening: the frame the kernel decodes
        want = ctx.bilateral_temporal(wide, k, radius=r, layers=layers, **sig(r))
        got = ctx.bilateral_temporal(packed, k, radius=r, layers=layers, **sig(r))
        for a, b in zip(got, want):
            assert same(a, b)
    want = ctx.bilateral_temporal(f32, k, radius=r, layers=layers, **sig(r))
    u8 = ctx.bilateral_temporal(f32, k, radius=r, layers=layers, out_dtype=np.uint8, **sig(r))
    f16 = ctx.bilateral_temporal(f32, k, radius=r, layers=layers, out_dtype=np.float16, **sig(r))
    for t in range(n):
        assert same(u8[t], ctx.pack_u8(want[t])) and same(f16[t], ctx.pack_f16(want[t]))


# ---- one full frame, no checker --------------------------------------------------------------------------------------------------
def test_1080p_equal_layers_give_the_mean_of_the_single_frame_results(ctx):
    # guides equal across the frames: every neighbour's weights and denominator are the single-frame filter's, so the output is
    # the mean of the three mid_bilateral_layers outputs (np_bilateral_temporal's known answer (b)) -- to fp32 rounding
    rng = np.random.default_rng(9)
    h, w, r = 1080, 1920, 8
    frames = frames_of(rng, 3, h, w)
    guides = layers_of(rng, 1, 2, h, w)[0]
    got = ctx.bilateral_temporal(frames, 1, 1, 1, radius=r, layers=[guides] * 3, **sig(r))[0]
    mean = sum(ctx.bilateral_layers(f, guides, r, **sig(r)).astype(np.float64) for f in frames) / 3
    e = rel_err(got, mean)
    print(f"1080p r=8 k=1 L=2: worst rel err against the mean of the single-frame outputs {e:.3e}")
    assert e < TOL


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_alone(ctx):
    h, w, n, L = 16, 64, 4, 2
    npix = h * w
    fr = [ctx.zeros(npix * 16 + 16) for _ in range(n)]
    ly = [ctx.zeros(npix * 4) for _ in range(n * L)]
    fill = np.full((h, w, 4), 7.0, np.float32)
    outs = [ctx.upload(fill) for _ in range(n)]
    Wfill = np.full((h, w, 8), 3.0, np.float32)
    dW = ctx.upload(Wfill)
    lib = mid.lib

    def P(radius=4, ss=2.0, sc=0.2, layout=mid.LAYOUT_TEXTURE, fmt=mid.FMT_RGBA32F, width=w, height=h):
        return mid.BilateralParams(width, height, ss, sc, radius, layout, fmt)

    def tbl(ptrs):
        return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)

    F, Lt, O = [b.ptr for b in fr], [b.ptr for b in ly], [b.ptr for b in outs]

    def temporal(p=None, frames=F, layers=Lt, n_layers=L, n_frames=n, k=1, first=0, count=n, out=O, out_fmt=mid.FMT_RGBA32F,
                 frames_tbl=True, out_tbl=True):
        return lib.mid_bilateral_temporal(ctx.handle, ctypes.byref(p or P()), tbl(frames) if frames_tbl else None,
                                          None if layers is None else tbl(layers), n_layers, n_frames, k, first, count,
                                          tbl(out) if out_tbl else None, out_fmt, None)

    assert temporal() == 0 and temporal(layers=None, n_layers=0) == 0          # the call itself is fine
    ctx.sync()
    for o in outs:
        lib.mid_memcpy_h2d(ctx.handle, o.ptr, fill.ctypes.data, fill.nbytes, None)
    ctx.sync()
    big = 11                                                                    # k = 5: 11 frames x 17 pointers = 187 > 176
    cases = {
        "radius 0": dict(p=P(radius=0)), "radius 25": dict(p=P(radius=25)), "sigma_s 0": dict(p=P(ss=0.0)), "sigma_c 0": dict(p=P(sc=0.0)),
        "format": dict(p=P(fmt=9)), "width 0": dict(p=P(width=0)), "layout": dict(p=P(layout=5)),
        "linear layout": dict(p=P(layout=mid.LAYOUT_LINEAR)), "linear layout, plain": dict(p=P(layout=mid.LAYOUT_LINEAR), layers=None, n_layers=0),
        "NULL frames": dict(frames_tbl=False), "NULL out": dict(out_tbl=False), "NULL frame": dict(frames=[F[0], None, F[2], F[3]]),
        "NULL layer": dict(layers=Lt[:3] + [None] + Lt[4:]), "NULL output": dict(out=[O[0], None, O[2], O[3]]),
        "17 layers": dict(n_layers=17, layers=Lt * 9), "-1 layers": dict(n_layers=-1), "plain with n_layers": dict(layers=None, n_layers=1),
        "k < 0": dict(k=-1), "first < 0": dict(first=-1, count=1), "count 0": dict(count=0), "range": dict(first=2, count=3),
        "n_frames 0": dict(n_frames=0, count=1), "out format": dict(out_fmt=7),
        "frame alignment": dict(p=P(fmt=mid.FMT_RGBA16F), frames=[F[0] + 4] + F[1:]),
        "output alignment": dict(out_fmt=mid.FMT_RGBA16F, out=[O[0] + 4] + O[1:]),
        "out is a frame": dict(out=[F[1]] + O[1:]), "out is a layer": dict(out=O[:3] + [Lt[2]]), "out twice": dict(out=[O[0], O[0], O[2], O[3]]),
        "pointer limit": dict(frames=[F[0]] * big, layers=[Lt[0]] * (big * 16), n_layers=16, n_frames=big, k=5, first=5, count=1),
    }
    for name, kw in cases.items():
        assert temporal(**kw) == 1, name                                       # MID_ERR_INVALID
        assert lib.mid_last_error(), name
    # a window the limit admits is not refused for its size (k = 4 with 16 layers: 9 x 17 = 153)
    assert temporal(frames=[F[0]] * 9, layers=[Lt[0]] * (9 * 16), n_layers=16, n_frames=9, k=4, first=4, count=1, out=O[:1]) == 0
    ctx.sync()
    lib.mid_memcpy_h2d(ctx.handle, O[0], fill.ctypes.data, fill.nbytes, None)
    pairs = {
        "pair: linear": lambda: lib.mid_bilateral_pair_accum(ctx.handle, ctypes.byref(P(layout=mid.LAYOUT_LINEAR)), F[0], F[1], dW.ptr, None),
        "pair: radius": lambda: lib.mid_bilateral_pair_accum(ctx.handle, ctypes.byref(P(radius=0)), F[0], F[1], dW.ptr, None),
        "pair: NULL target": lambda: lib.mid_bilateral_pair_accum(ctx.handle, ctypes.byref(P()), None, F[1], dW.ptr, None),
        "pair: NULL W": lambda: lib.mid_bilateral_pair_accum(ctx.handle, ctypes.byref(P()), F[0], F[1], None, None),
        "pair: alignment": lambda: lib.mid_bilateral_pair_accum(ctx.handle, ctypes.byref(P(fmt=mid.FMT_RGBA16F)), F[0] + 4, F[1], dW.ptr, None),
        "layers pair: linear": lambda: lib.mid_bilateral_layers_pair_accum(ctx.handle, ctypes.byref(P(layout=mid.LAYOUT_LINEAR)), Lt[0], Lt[1], F[0], dW.ptr, None),
        "layers pair: NULL guide": lambda: lib.mid_bilateral_layers_pair_accum(ctx.handle, ctypes.byref(P()), None, Lt[1], F[0], dW.ptr, None),
        "layers pair: NULL input": lambda: lib.mid_bilateral_layers_pair_accum(ctx.handle, ctypes.byref(P()), Lt[0], Lt[1], None, dW.ptr, None),
        "layers pair: alignment": lambda: lib.mid_bilateral_layers_pair_accum(ctx.handle, ctypes.byref(P(fmt=mid.FMT_RGBA16F)), Lt[0], Lt[1], F[0] + 4, dW.ptr, None),
    }
    for name, call in pairs.items():
        assert call() == 1, name
    ctx.sync()
    for o in outs:
        assert np.array_equal(ctx.download(o, (h, w, 4), np.float32), fill)
    assert np.array_equal(ctx.download(dW, (h, w, 8), np.float32), Wfill)
    for i in range(n):                                                          # (no refused call wrote a frame or a layer either)
        assert not ctx.download(fr[i], (h, w, 4), np.float32).any()
