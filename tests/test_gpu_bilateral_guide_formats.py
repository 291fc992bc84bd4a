"""GPU suite: half and float guide layers in the layer-guided bilateral family (MID_FMT_WITH_GUIDE), in every kernel class of
bilateral_temporal.hip -- radii 4, 8, 10, 20 (tuned), 5 (run-time radius), 18 (per pixel) -- at the shapes of
test_gpu_kernel_bits.py: 45 x 133 (partial tiles, seams) and 74 x 148 (a tile whose halo lies inside the frame: the opaque form
of the tap loop), opaque and translucent frames, three frames, two layers.

The four forms: fused (bilateral_layers), accumulate (bilateral_layers_accum), pair accumulate (bilateral_layers_pair_accum),
temporal (bilateral_temporal, n = 3, k = 1).  What is asserted, in this order: a float32 guide c / 255 gives the BITS of the RGBA8
guide c; a float16 guide the bits of the float32 guide it widens to; guides outside [0, 1] match the float64 checker
(np_bilateral_temporal.py) within the bilateral tolerance; non-finite guide texels follow IEEE arithmetic; fused == chain,
k = 0 == single frame, pair with equal guides == accumulate; the frame pipelines give the resident calls' bits and keep their
layer ring right between guide formats; every refusal of the header, with the outputs untouched.
"""
import ctypes

import numpy as np
import pytest

import guide_format_inputs as gi
import image_denoising_filter_amd as mid
import np_bilateral_temporal as chk
from conftest import rel_err
from test_gpu_kernel_bits import BIL, BIL_IN, SC, SS, frame, guide

pytestmark = pytest.mark.gpu

RADII = (4, 8, 10, 20, 5, 18)
SHAPED = [(BIL, r) for r in RADII] + [(BIL_IN, r) for r in (8, 10, 20)]
IDS = [f"{'edge' if s == BIL else 'interior'}-r{r}" for s, r in SHAPED]
KINDS = pytest.mark.parametrize("translucent", [False, True], ids=["opaque", "translucent"])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def four_forms(ctx, fr, gl, r, ss=SS, sc=SC):
    """The four forms on frames fr[0..2] and guides gl[frame][layer]: a list of arrays."""
    Z = np.zeros(fr[0].shape[:2] + (8,), np.float32)
    return [ctx.bilateral_layers(fr[0], gl[0], r, ss, sc),
            ctx.bilateral_layers_accum(fr[0], gl[0][0], Z, r, ss, sc),
            ctx.bilateral_layers_pair_accum(gl[0][0], gl[1][0], fr[1], Z, r, ss, sc),
            *ctx.bilateral_temporal(fr, 1, radius=r, sigma_s=ss, sigma_c=sc, layers=gl)]


def assert_all_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), f"{what}: form/output {i} differs"


def as_f32(g8, alpha):
    """The float32 guide with rgb = the IEEE quotient c / 255 that decode_rgba8 forms, and `alpha` in the fourth channel."""
    g = g8.astype(np.float32) / np.float32(255)
    g[..., 3] = alpha
    return g


# ---- 1. RGBA8 identity ---------------------------------------------------------------------------------------------------------
@KINDS
@pytest.mark.parametrize("shape,r", SHAPED, ids=IDS)
def test_float_guide_c_over_255_has_the_bits_of_the_rgba8_guide(ctx, shape, r, translucent):
    fr = [frame(shape, f, translucent) for f in range(3)]
    g8 = [[guide(shape, f, l) for l in range(2)] for f in range(3)]
    want = four_forms(ctx, fr, g8, r)
    h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    odd = np.where((x + y) % 7 == 0, np.float32(np.nan), (x - y).astype(np.float32))     # any alpha, NaN included: it is ignored
    for alpha in (np.float32(0.25), odd):
        g32 = [[as_f32(g, alpha) for g in ls] for ls in g8]
        assert_all_same(four_forms(ctx, fr, g32, r), want, f"alpha {'0.25' if alpha is not odd else 'pattern'}")


@KINDS
@pytest.mark.parametrize("dt", [np.uint8, np.float16], ids=["u8-frames", "f16-frames"])
def test_rgba8_identity_with_packed_frames(ctx, dt, translucent):
    fr = [frame(BIL, f, translucent, dt) for f in range(3)]
    g8 = [[guide(BIL, f, l) for l in range(2)] for f in range(3)]
    g32 = [[as_f32(g, 0.5) for g in ls] for ls in g8]
    assert_all_same(four_forms(ctx, fr, g32, 8), four_forms(ctx, fr, g8, 8), np.dtype(dt).name)


# ---- 2. half identity ----------------------------------------------------------------------------------------------------------
@KINDS
@pytest.mark.parametrize("shape,r", SHAPED, ids=IDS)
def test_half_guide_has_the_bits_of_the_float_guide_it_widens_to(ctx, shape, r, translucent):
    fr = [frame(shape, f, translucent) for f in range(3)]
    g16 = [ls[:2] for ls in gi.render_layers(shape, 3, np.float16)]                      # normals and albedo
    g32 = [[g.astype(np.float32) for g in ls] for ls in g16]
    want = four_forms(ctx, fr, g32, r, gi.SIGMA_S, gi.SIGMA_C)
    assert_all_same(four_forms(ctx, fr, g16, r, gi.SIGMA_S, gi.SIGMA_C), want, "f16 guides")


# ---- 3. against the float64 checker ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker_case():
    """Frames, float32 layers and the float64 reference of every radius class, computed once."""
    fr = gi.hdr_frames(BIL, 3, translucent=True)
    gl = gi.render_layers(BIL, 3, np.float32)
    assert gi.max_guide_ratio(gl) <= 16.0
    return fr, gl, {}


@pytest.mark.parametrize("dt", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("r", RADII)
def test_render_layers_match_the_float64_checker(ctx, checker_case, r, dt):
    fr, gl32, cache = checker_case
    gl = gl32 if dt == np.float32 else gi.render_layers(BIL, 3, np.float16)
    key = (r, np.dtype(dt).name)
    if key not in cache:
        cache[key] = chk.bilateral_temporal(fr, 1, r, gi.SIGMA_S, gi.SIGMA_C, layers=gl)
    got = ctx.bilateral_temporal(fr, 1, radius=r, sigma_s=gi.SIGMA_S, sigma_c=gi.SIGMA_C, layers=gl)
    errs = [rel_err(g, x) for g, x in zip(got, cache[key])]
    single = rel_err(ctx.bilateral_layers(fr[1], gl[1], r, gi.SIGMA_S, gi.SIGMA_C),
                     chk.bilateral_temporal(fr[1:2], 0, r, gi.SIGMA_S, gi.SIGMA_C, layers=gl[1:2])[0])
    print(f"r={r} {np.dtype(dt).name} guides (max |g|/sigma_c {gi.max_guide_ratio(gl):.1f}): worst rel err temporal {max(errs):.3e}, single frame {single:.3e}")
    assert max(errs) < gi.TOL and single < gi.TOL


# ---- 4. non-finite guide texels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("r", [8, 5, 18])
def test_inf_and_nan_guide_texels_follow_ieee(ctx, r, dt):
    shape = BIL_IN
    fr = gi.hdr_frames(shape, 3, seed=21)
    gl = [ls[:2] for ls in gi.render_layers(shape, 3, dt, seed=22)]
    gl[1][0][40, 100, 1] = np.inf                                                   # an interior tile (rows 32..47, columns 64..127)
    gl[1][1][36, 80, 2] = np.nan
    kw = dict(sigma_s=gi.SIGMA_S, sigma_c=gi.SIGMA_C)
    got = ctx.bilateral_temporal(fr, 1, radius=r, layers=gl, **kw)
    want = chk.bilateral_temporal(fr, 1, r, gi.SIGMA_S, gi.SIGMA_C, layers=gl)
    for t in range(3):
        nan = np.isnan(want[t])
        assert np.array_equal(np.isnan(got[t]), nan), t
        assert nan.any() and not nan.all()
        assert rel_err(got[t][~nan], want[t][~nan]) < gi.TOL
        # the fused call and its chain of accumulate calls + normalize: the same bits, NaNs included
        W = np.zeros(shape + (8,), np.float32)
        for f in chk.window(3, t, 1):
            for lt, lf in zip(gl[t], gl[f]):
                W = ctx.bilateral_layers_pair_accum(lt, lf, fr[f], W, r, **kw)
        assert same(got[t], ctx.normalize(W)), t
    # single frame: the Inf texel's own pixel is poisoned (Inf - Inf), its neighbours see weight 0 from it
    one = ctx.bilateral_layers(fr[1], gl[1][:1], r, **kw)
    assert np.isnan(one[40, 100]).all() and np.isnan(one).sum() == 4
    W = ctx.bilateral_layers_accum(fr[1], gl[1][0], np.zeros(shape + (8,), np.float32), r, **kw)
    assert same(one, ctx.normalize(W))


# ---- 5. chain and k = 0 identities for the new formats -------------------------------------------------------------------------------
@KINDS
@pytest.mark.parametrize("dt", [np.float32, np.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("shape,r", SHAPED, ids=IDS)
def test_chain_k0_and_equal_guide_identities(ctx, shape, r, dt, translucent):
    fr = [frame(shape, f, translucent) for f in range(3)]
    gl = [ls[:2] for ls in gi.render_layers(shape, 3, dt)]
    kw = dict(sigma_s=gi.SIGMA_S, sigma_c=gi.SIGMA_C)
    fused = ctx.bilateral_temporal(fr, 1, radius=r, layers=gl, **kw)
    for t in range(3):
        W = np.zeros(shape + (8,), np.float32)
        for f in chk.window(3, t, 1):
            for lt, lf in zip(gl[t], gl[f]):
                W = ctx.bilateral_layers_pair_accum(lt, lf, fr[f], W, r, **kw)
        assert same(fused[t], ctx.normalize(W)), t
    if r == 8:                                       # (+ pack)
        for odt, pack in ((np.uint8, ctx.pack_u8), (np.float16, ctx.pack_f16)):
            packed = ctx.bilateral_temporal(fr, 1, radius=r, layers=gl, out_dtype=odt, **kw)
            assert all(same(p, pack(f)) for p, f in zip(packed, fused))
    k0 = ctx.bilateral_temporal(fr, 0, radius=r, layers=gl, **kw)
    for t in range(3):
        assert same(k0[t], ctx.bilateral_layers(fr[t], gl[t], r, gi.SIGMA_S, gi.SIGMA_C)), t
    W0 = np.random.default_rng(r).random(shape + (8,), dtype=np.float32)
    want = ctx.bilateral_layers_accum(fr[2], gl[2][1], W0, r, gi.SIGMA_S, gi.SIGMA_C)
    assert not np.array_equal(want, W0)
    assert same(ctx.bilateral_layers_pair_accum(gl[2][1], gl[2][1], fr[2], W0, r, **kw), want)
    assert same(ctx.bilateral_layers_pair_accum(gl[2][1].copy(), gl[2][1], fr[2], W0, r, **kw), want)


# ---- 6. pipelines --------------------------------------------------------------------------------------------------------------
GUARD, GUARD_BYTE = 64, 0xA5


def run_pipeline(ctx, temporal, frames, layers, out_dt, pinned, r=8, k=1):
    """mid_sequence_bilateral[_temporal] on host buffers of this test's own, every output followed by GUARD bytes: the outputs,
    after checking that the guards kept their bits."""
    n, (h, w) = len(frames), frames[0].shape[:2]
    flat = [l for ls in layers for l in ls]
    nbytes = h * w * 4 * np.dtype(out_dt).itemsize
    fmt = mid.api._guide_fmt(mid.api._fmt_of(frames[0]), flat, "test")
    hin = hlay = hout = None
    try:
        if pinned:
            hin, hlay, hout = mid.PinnedFrames(ctx, frames), mid.PinnedFrames(ctx, flat), mid.PinnedFrames(ctx, n, nbytes + GUARD)
            for p in hout.ptrs:
                ctypes.memset(p, GUARD_BYTE, nbytes + GUARD)
            pin, play, pout = hin.ptrs, hlay.ptrs, hout.ptrs
        else:
            bufs = [np.full(nbytes + GUARD, GUARD_BYTE, np.uint8) for _ in range(n)]
            pin, play, pout = [f.ctypes.data for f in frames], [l.ctypes.data for l in flat], [b.ctypes.data for b in bufs]
        if temporal:
            ctx.sequence_bilateral_temporal_pinned(pin, pout, w, h, fmt, k, 0, n, r, gi.SIGMA_S, gi.SIGMA_C, play, len(layers[0]), True, out_dt)
        else:
            ctx.sequence_bilateral_pinned(pin, pout, w, h, fmt, r, gi.SIGMA_S, gi.SIGMA_C, "texture", play, len(layers[0]), True, out_dt)
        outs = []
        for i in range(n):
            raw = np.ctypeslib.as_array((ctypes.c_uint8 * (nbytes + GUARD)).from_address(pout[i])).copy()
            assert (raw[nbytes:] == GUARD_BYTE).all(), f"the guard bytes behind output {i} were written"
            outs.append(raw[:nbytes].view(out_dt).reshape(h, w, 4))
        return outs
    finally:
        for b in (hin, hlay, hout):
            if b is not None:
                b.free()


def resident(ctx, temporal, frames, layers, out_dt, r=8, k=1):
    kw = dict(sigma_s=gi.SIGMA_S, sigma_c=gi.SIGMA_C)
    if temporal:
        return ctx.bilateral_temporal(frames, k, radius=r, layers=layers, out_dtype=out_dt, **kw)
    pack = {np.float32: lambda a: a, np.float16: ctx.pack_f16, np.uint8: ctx.pack_u8}[out_dt]
    return [pack(ctx.bilateral_layers(f, ls, r, gi.SIGMA_S, gi.SIGMA_C)) for f, ls in zip(frames, layers)]


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "pageable"])
@pytest.mark.parametrize("dt", [np.float32, np.float16], ids=["f32-layers", "f16-layers"])
@pytest.mark.parametrize("temporal", [False, True], ids=["sequence_bilateral", "sequence_bilateral_temporal"])
def test_pipelines_give_the_resident_bits(ctx, temporal, dt, pinned):
    n, shape = 5, BIL
    frames = gi.hdr_frames(shape, n, seed=31, translucent=True)
    layers = [ls[:2] for ls in gi.render_layers(shape, n, dt, seed=32)]
    for out_dt in (np.float32, np.float16, np.uint8):
        got = run_pipeline(ctx, temporal, frames, layers, out_dt, pinned)
        assert_all_same(got, resident(ctx, temporal, frames, layers, out_dt), np.dtype(out_dt).name)
    # and through the public wrappers, which pick the guide field from the dtype
    seq = ctx.sequence_bilateral_temporal(frames, 1, radius=8, sigma_s=gi.SIGMA_S, sigma_c=gi.SIGMA_C, layers=layers, pinned=pinned, pinned_out=pinned)[0] \
        if temporal else ctx.sequence_bilateral(frames, 8, gi.SIGMA_S, gi.SIGMA_C, layers=layers, pinned=pinned, pinned_out=pinned)[0]
    assert_all_same(seq, resident(ctx, temporal, frames, layers, np.float32), "wrapper")


@pytest.mark.parametrize("order", ["u8-then-f32", "f32-then-u8"])
@pytest.mark.parametrize("temporal", [False, True], ids=["sequence_bilateral", "sequence_bilateral_temporal"])
def test_layer_ring_between_guide_formats(temporal, order):
    """One context of its own (the ring starts empty): RGBA8 layers and float32 layers alternate, so the ring must grow from
    4 to 16 bytes per texel -- or be kept at 16 -- and either way hold whole layers."""
    n, shape = 5, BIL
    frames = gi.hdr_frames(shape, n, seed=41)
    f32 = [ls[:2] for ls in gi.render_layers(shape, n, np.float32, seed=42)]
    u8 = [[guide(shape, f, l) for l in range(2)] for f in range(n)]
    seq = [u8, f32, u8] if order == "u8-then-f32" else [f32, u8, f32]
    with mid.Context(0) as c:
        for layers in seq:
            for pinned in (True, False):
                got = run_pipeline(c, temporal, frames, layers, np.float32, pinned)
                assert_all_same(got, resident(c, temporal, frames, layers, np.float32), f"{layers[0][0].dtype} layers")


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_alone(ctx):
    h, w, n, L = 16, 64, 3, 2
    npix = h * w
    G = mid.api.fmt_with_guide
    F32, U8, F16 = mid.FMT_RGBA32F, mid.FMT_RGBA8, mid.FMT_RGBA16F
    fr = [ctx.zeros(npix * 16) for _ in range(n)]
    ly = [ctx.zeros(npix * 16 + 16) for _ in range(n * L)]
    fill, Wfill = np.full((h, w, 4), 7.0, np.float32), np.full((h, w, 8), 3.0, np.float32)
    outs, dW = [ctx.upload(fill) for _ in range(n)], ctx.upload(Wfill)
    lib, H = mid.lib, ctx.handle
    Fp, Lp, Op = [b.ptr for b in fr], [b.ptr for b in ly], [b.ptr for b in outs]

    def P(fmt, radius=4):
        return ctypes.byref(mid.BilateralParams(w, h, 2.0, 0.2, radius, mid.LAYOUT_TEXTURE, fmt))

    def N(fmt):
        return ctypes.byref(mid.NlmParams(w, h, 0.5, -2, 3, -1, 2, fmt))

    def tbl(ptrs):
        return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)

    def temporal(fmt, layers=Lp, n_layers=L):
        return lib.mid_bilateral_temporal(H, P(fmt), tbl(Fp), None if layers is None else tbl(layers), n_layers, n, 1, 0, n, tbl(Op), F32, None)

    # the calls themselves are fine with a guide field (and 1 + MID_FMT_RGBA8 is RGBA8 spelled out)
    for g in (F32, F16, U8):
        assert temporal(G(F32, g)) == 0, mid.lib.mid_last_error()
        assert lib.mid_bilateral_layers(H, P(G(F32, g)), Fp[0], tbl(Lp[:L]), L, Op[0], None) == 0
        assert lib.mid_bilateral_layers_accum(H, P(G(F32, g)), Fp[0], Lp[0], dW.ptr, None) == 0
        assert lib.mid_bilateral_layers_pair_accum(H, P(G(F32, g)), Lp[0], Lp[1], Fp[0], dW.ptr, None) == 0
    ctx.sync()
    for o in outs:
        lib.mid_memcpy_h2d(H, o.ptr, fill.ctypes.data, fill.nbytes, None)
    lib.mid_memcpy_h2d(H, dW.ptr, Wfill.ctypes.data, Wfill.nbytes, None)
    ctx.sync()

    g32, g16 = G(F32, F32), G(F32, F16)
    host = [np.zeros((h, w, 4), np.float32) for _ in range(n)]
    hostl = [np.zeros((h, w, 4), np.float32) for _ in range(n * L)]
    hout = [np.full((h, w, 4), 7.0, np.float32) for _ in range(n)]
    hp = lambda arrs: tbl([a.ctypes.data for a in arrs])
    t3 = (ctypes.c_float * 3)()
    cases = {
        # entry points that read no guide layers of the bilateral family
        "bilateral": lambda: lib.mid_bilateral(H, P(g32), Fp[0], Op[0], None),
        "bilateral, RGBA8 spelled out": lambda: lib.mid_bilateral(H, P(G(F32, U8)), Fp[0], Op[0], None),
        "bilateral linear": lambda: lib.mid_bilateral(H, ctypes.byref(mid.BilateralParams(w, h, 2.0, 0.2, 4, mid.LAYOUT_LINEAR, g32)), Fp[0], Op[0], None),
        "bilateral_batch": lambda: lib.mid_bilateral_batch(H, P(g16), tbl(Fp), tbl(Op), n, None),
        "bilateral_pair_accum": lambda: lib.mid_bilateral_pair_accum(H, P(g32), Fp[0], Fp[1], dW.ptr, None),
        "bilateral_temporal, plain": lambda: temporal(g32, layers=None, n_layers=0),
        "sequence_bilateral, plain": lambda: lib.mid_sequence_bilateral(H, P(g32), hp(host), n, None, 0, hp(hout), F32, 1, t3),
        "sequence_bilateral_temporal, plain": lambda: lib.mid_sequence_bilateral_temporal(H, P(g32), hp(host), n, None, 0, 1, 0, n, hp(hout), F32, 1, t3),
        "nlm_accum": lambda: lib.mid_nlm_accum(H, N(g32), Fp[0], Fp[1], dW.ptr, None),
        "nlm_temporal": lambda: lib.mid_nlm_temporal(H, N(g16), tbl(Fp), n, 1, 0, n, tbl(Op), None),
        "nlm_layers_accum": lambda: lib.mid_nlm_layers_accum(H, N(g32), Fp[0], Lp[0], dW.ptr, None),
        "nlm_layers": lambda: lib.mid_nlm_layers(H, N(g32), Fp[0], tbl(Lp[:L]), L, Op[0], None),
        "nlm_layers_pair_accum": lambda: lib.mid_nlm_layers_pair_accum(H, N(g16), Lp[0], Lp[1], Fp[0], dW.ptr, None),
        "nlm_layers_temporal": lambda: lib.mid_nlm_layers_temporal(H, N(g32), tbl(Fp), tbl(Lp), L, n, 1, 0, n, tbl(Op), F32, None),
        "sequence_nlm_layers": lambda: lib.mid_sequence_nlm_layers(H, N(g32), hp(host), n, hp(hostl), L, hp(hout), F32, 1, t3),
        "sequence_nlm_layers_temporal": lambda: lib.mid_sequence_nlm_layers_temporal(H, N(g32), hp(host), n, hp(hostl), L, 1, 0, n, hp(hout), F32, 1, t3),
        # unknown guide codes, bits above the guide field, and the formats that were always invalid
        "guide code 4": lambda: temporal(F32 | (4 << 8)),
        "guide code 255": lambda: lib.mid_bilateral_layers(H, P(F32 | (255 << 8)), Fp[0], tbl(Lp[:L]), L, Op[0], None),
        "bits above 15": lambda: temporal(g32 | (1 << 16)),
        "negative": lambda: temporal(-1),
        "format 7": lambda: temporal(7), "format 9": lambda: temporal(9),
        "format 7, layers": lambda: lib.mid_bilateral_layers(H, P(7), Fp[0], tbl(Lp[:L]), L, Op[0], None),
        "format 9, accum": lambda: lib.mid_bilateral_layers_accum(H, P(9), Fp[0], Lp[0], dW.ptr, None),
        "frames 7 with a guide": lambda: temporal(7 | (1 << 8)),
        "sequence_bilateral, guide code 9": lambda: lib.mid_sequence_bilateral(H, P(F32 | (9 << 8)), hp(host), n, hp(hostl), L, hp(hout), F32, 1, t3),
        "sequence_bilateral_temporal, guide code 9": lambda: lib.mid_sequence_bilateral_temporal(H, P(F32 | (9 << 8)), hp(host), n, hp(hostl), L, 1, 0, n, hp(hout), F32, 1, t3),
        # alignment of the guide layers: RGBA16F 8 bytes, RGBA32F 16 bytes
        "f16 guide at +4, temporal": lambda: temporal(g16, layers=[Lp[0] + 4] + Lp[1:]),
        "f32 guide at +8, temporal": lambda: temporal(g32, layers=Lp[:3] + [Lp[3] + 8] + Lp[4:]),
        "f32 guide at +4, layers": lambda: lib.mid_bilateral_layers(H, P(g32), Fp[0], tbl([Lp[0], Lp[1] + 4]), L, Op[0], None),
        "f16 guide at +4, layers": lambda: lib.mid_bilateral_layers(H, P(g16), Fp[0], tbl([Lp[0] + 4, Lp[1]]), L, Op[0], None),
        "f32 guide at +8, accum": lambda: lib.mid_bilateral_layers_accum(H, P(g32), Fp[0], Lp[0] + 8, dW.ptr, None),
        "f16 guide at +4, accum": lambda: lib.mid_bilateral_layers_accum(H, P(g16), Fp[0], Lp[0] + 4, dW.ptr, None),
        "f32 target guide at +8, pair": lambda: lib.mid_bilateral_layers_pair_accum(H, P(g32), Lp[0] + 8, Lp[1], Fp[0], dW.ptr, None),
        "f16 neighbour guide at +4, pair": lambda: lib.mid_bilateral_layers_pair_accum(H, P(g16), Lp[0], Lp[1] + 4, Fp[0], dW.ptr, None),
    }
    for name, call in cases.items():
        assert call() == 1, name                                                  # MID_ERR_INVALID
        assert lib.mid_last_error(), name
    for name in ("nlm_layers_accum", "nlm_layers", "nlm_layers_pair_accum", "nlm_layers_temporal", "sequence_nlm_layers", "sequence_nlm_layers_temporal"):
        assert cases[name]() == 1 and b"RGBA8 guide layers only" in lib.mid_last_error(), name
    # an RGBA16F guide at +8 and RGBA8 guides at +4 are aligned for what they are
    assert temporal(g16, layers=[Lp[0] + 8] + Lp[1:]) == 0 and temporal(F32, layers=[Lp[0] + 4] + Lp[1:]) == 0
    ctx.sync()
    for o in outs:
        lib.mid_memcpy_h2d(H, o.ptr, fill.ctypes.data, fill.nbytes, None)
    ctx.sync()
    for name, call in cases.items():
        assert call() == 1, name
    ctx.sync()
    for o in outs:
        assert np.array_equal(ctx.download(o, (h, w, 4), np.float32), fill)
    assert np.array_equal(ctx.download(dW, (h, w, 8), np.float32), Wfill)
    assert all(np.array_equal(o, np.full((h, w, 4), 7.0, np.float32)) for o in hout)


def test_python_refuses_mixed_and_nlm_float_layers(ctx):
    shape = (20, 70)
    fr = [frame(shape, f, False) for f in range(2)]
    u8 = [[guide(shape, f, l) for l in range(2)] for f in range(2)]
    f32 = [[as_f32(g, 1.0) for g in ls] for ls in u8]
    mixed = [[u8[0][0], f32[0][1]], u8[1]]
    Z = np.zeros(shape + (8,), np.float32)
    for call in (lambda: ctx.bilateral_layers(fr[0], mixed[0], 4), lambda: ctx.bilateral_temporal(fr, 1, radius=4, layers=mixed),
                 lambda: ctx.bilateral_layers_pair_accum(u8[0][0], f32[1][0], fr[1], Z, 4),
                 lambda: ctx.sequence_bilateral(fr, 4, layers=mixed), lambda: ctx.sequence_bilateral_temporal(fr, 1, radius=4, layers=[u8[0], f32[1]])):
        with pytest.raises(ValueError):
            call()
    win = dict(search=(-2, 3), patch=(-1, 2))
    for call in (lambda: ctx.nlm_layers(fr[0], f32[0], 0.5, **win), lambda: ctx.nlm_layers_accum(fr[0], f32[0][0], Z, 0.5, **win),
                 lambda: ctx.nlm_layers_pair_accum(f32[0][0], f32[1][0], fr[1], Z, 0.5, **win),
                 lambda: ctx.nlm_layers_temporal(fr, f32, 1, hparam=0.5, **win), lambda: ctx.sequence_nlm_layers(fr, f32, hparam=0.5, **win),
                 lambda: ctx.sequence_nlm_layers_temporal(fr, f32, 1, hparam=0.5, **win),
                 lambda: ctx.nlm_layers_temporal(fr, [[g.astype(np.float16) for g in ls] for ls in f32], 1, hparam=0.5, **win)):
        with pytest.raises((TypeError, ValueError)):
            call()
