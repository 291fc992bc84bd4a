"""Joint layer-guided NLM (mid_nlm_joint, csrc/nlm_joint.hip; include/mi_denoise.h, section a4f) where its kernels go wrong
unnoticed and where the file is NOT a copy of the layered one: the 32-row tiles and 4-row waves of the 2-, 3- and 4-layer classes
(frames smaller than a tile, a wave or the window; frames that end at, or one past, a wave or tile seam of either tile height;
nothing written behind the frame in any output format); every tile count from 1 to 17 and a few larger, ragged grids (the XCD remap
of the tile index over cdiv(h, 32) x cdiv(w, VW)); HDR colours with h from 0.02 to 50 and h_0 / h_l from 1/2500 to 2500, where
D = D_0 + sum r_l D_l is no integer any more; NaN and +-Inf texels in general and in opaque tiles; the guide's alpha byte and the
frames outside [first - k, first + count + k), which the contract does not read.

Every comparison is with the float64 checker (np_nlm_joint; tests/test_nlm_joint_checker_edges.py anchors it at these places) at
the header's 2e-5 * max(1, |ref|), with the header's bit identities (one layer is mid_nlm_layers_temporal; a packed output is
mid_pack_* of the float result), or with the bytes a buffer held before the call.

Windows: A = 21x21 / 7x7 (58 valid columns a tile), B = 14x14 / 6x6 (59), U = 7x7 / 3x3 (untuned: one thread per pixel).  Guides wrap
at 256: a ramp that saturates at 255 on a wide frame is flat, and every weight 1."""
import ctypes

import numpy as np
import pytest

import image_denoising_filter_amd as mid
import np_nlm_joint as chk
from conftest import synth_hdr
from test_gpu_nlm_joint import BIG, HS, ODD, TOL, WIN, bits, frames_of, rel_err, same
from test_gpu_nlm_layers import NLM_CFGS
from test_gpu_nlm_layers_edges import _tile_cases, same_masks_and_values

# (the checker shares the search offsets out over threads, and NumPy's error state is per thread: np.errstate does not reach them)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered:RuntimeWarning")]

VW = {"21x21": 58, "14x14": 59}             # output columns of a strip-kernel tile: 64 - (patch width - 1)
TILE_H = 32                                 # tile rows of the 2-, 3- and 4-layer classes (64 with one layer)
STRIP = [(win, L) for win in ("21x21", "14x14") for L in (1, 2, 3, 4)]
PER_PIXEL = [("21x21", 5), ("7x7", 2)]      # more than four layers; an untuned window
CLASSES = STRIP + PER_PIXEL
FMT = {np.dtype(np.uint8): mid.FMT_RGBA8, np.dtype(np.float16): mid.FMT_RGBA16F, np.dtype(np.float32): mid.FMT_RGBA32F}

TINY = [(1, 1), (1, 40), (40, 1), (2, 70), (70, 2), (9, 9), (3, 5)]
SEAMS_32 = [(4, 58), (5, 58), (31, 57), (32, 58), (32, 59), (33, 59), (33, 60), (36, 58), (37, 58), (64, 116), (65, 117), (96, 118),
            (97, 119)]
SEAMS_64 = [(63, 57), (64, 58), (64, 59), (65, 59), (65, 60), (128, 116), (129, 119)]
SHAPES = TINY + SEAMS_32 + SEAMS_64


def cls_id(c):
    return f"{c[0]}-L{c[1]}"


def shape_id(s):
    return f"{s[0]}x{s[1]}"


def wrap_guides(shape, n, L, seed=0, sparse=False):
    """test_gpu_nlm_joint.big_inputs' guides for any shape and layer count: ramps of slope 1 or 2 in x and in y, a few codes apart
    from frame to frame, that WRAP at 256, with 0..3 codes of texture on top, so that many offsets carry a weight strictly between
    0 and 1 at h = 0.1 .. 1; `seed` moves every layer's channels by a phase of its own.  sparse: the texture is one code on one
    texel in 16 instead -- a patch distance of a few codes^2, which a layer of h = 0.02 still weighs strictly between 0 and 1
    (one code^2 there is a factor exp(-0.038)); with the full texture such a layer matches at the centre alone."""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    ph = np.random.default_rng(seed).integers(0, 256, (L, 3)) if seed else np.zeros((L, 3), np.int64)

    def texture(f, l, c):
        t = x * 7 + y * 13 + f * 5 + l * 3 + c
        return (t % 16 == 0).astype(np.int64) if sparse else t % 4

    return [[np.stack([(x * (1 + l % 2) + y * (1 + l // 2 % 2) + 3 * f + 20 * l + 10 * c + ph[l, c] + texture(f, l, c)) % 256
                       for c in range(3)] + [np.full_like(x, 255)], -1).astype(np.uint8) for l in range(L)] for f in range(n)]


def raw_joint(ctx, frames, layers, hs, k, first, count, win, before, hparam=0.5):
    """mid_nlm_joint through the C entry point into output buffers that hold `before` (one host array per output, at least the
    frame's size; its dtype is the output format): what the buffers hold afterwards."""
    search, patch = WIN[win] if isinstance(win, str) else win
    h, w = frames[0].shape[:2]
    n, L = len(frames), len(layers[0])
    d_fr = [ctx.upload(f) for f in frames]
    d_l = [ctx.upload(g) for ls in layers for g in ls]
    d_out = [ctx.upload(b) for b in before]
    assert len(before) == count and all(b.nbytes >= h * w * 4 * b.dtype.itemsize for b in before)
    p = mid.NlmParams(w, h, hparam, search[0], search[1], patch[0], patch[1], FMT[frames[0].dtype])
    rc = mid.lib.mid_nlm_joint(ctx.handle, ctypes.byref(p), (ctypes.c_float * L)(*hs), (ctypes.c_void_p * n)(*[d.ptr for d in d_fr]),
                               (ctypes.c_void_p * (n * L))(*[d.ptr for d in d_l]), L, n, k, first, count,
                               (ctypes.c_void_p * count)(*[d.ptr for d in d_out]), FMT[before[0].dtype], None)
    assert rc == 0, mid.lib.mid_last_error()
    ctx.sync()
    return [ctx.download(d, b.shape, b.dtype) for d, b in zip(d_out, before)]


def nan_frame(shape):
    return np.full(shape + (4,), np.nan, np.float32)


def check(what, got, want):
    """Every pixel of every output within TOL of the checker (a NaN the call left or made fails it)."""
    assert len(got) == len(want)
    err = max(rel_err(g, w) for g, w in zip(got, want))
    print(f"{what}: {err:.2e}")
    assert err < TOL, (what, err)
    return err


# ---- 2. tiny frames, seams of both tile heights, nothing written beyond the frame ---------------------------------------------
@pytest.mark.parametrize("cls", CLASSES, ids=cls_id)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_tiny_and_seam_frames(ctx, shape, cls):
    win, L = cls
    search, patch = WIN[win]
    case = SHAPES.index(shape) + CLASSES.index(cls)
    translucent = case % 2 == 1                 # alpha 0.5 in 5 % of the texels: the general form of the weight sums
    fr = frames_of(shape, 1, translucent=translucent, seed=100 + case)
    gl = wrap_guides(shape, 1, L, seed=200 + case)
    got = ctx.nlm_joint(fr, gl, HS[:L], 0, search=search, patch=patch)
    check(f"part 2 {win} L={L} {shape_id(shape)} {'translucent' if translucent else 'opaque'}", got,
          chk.nlm_joint(fr, gl, HS[:L], 0, search, patch))
    if L == 1:                                  # identity 1
        assert same(got[0], ctx.nlm_layers_temporal(fr, gl, 0, hparam=HS[0], search=search, patch=patch)[0]), (cls, shape)


GUARD_CLASSES = [(win, L) for win in ("21x21", "14x14") for L in (1, 2, 4)] + [("7x7", 2)]


@pytest.mark.parametrize("cls", GUARD_CLASSES, ids=cls_id)
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_nothing_is_written_beyond_the_frame(ctx, shape, cls):
    # The last tile row has rows at and below the frame's end -- whole waves of 4 (8) rows, and the tail of the wave that holds row
    # h - 1 -- and the last tile column has lanes right of it; a write from one of them lands in the next row or behind the buffer,
    # where no comparison of the h x w result sees it.  So the output gets GUARD more rows of random bits, a whole tile's height in
    # the output's own texel size, which the call must leave alone.
    GUARD = 64
    win, L = cls
    search, patch = WIN[win]
    h, w = shape
    case = SHAPES.index(shape) + GUARD_CLASSES.index(cls)
    rng = np.random.default_rng(3000 * h + w + case)
    fr = frames_of(shape, 2, translucent=True, seed=300 + case)
    gl = wrap_guides(shape, 2, L, seed=400 + case)
    plain = ctx.nlm_joint(fr, gl, HS[:L], 1, first=1, count=1, search=search, patch=patch)[0]
    check(f"part 2 guard {win} L={L} {shape_id(shape)}", [plain], chk.nlm_joint(fr, gl, HS[:L], 1, search, patch, first=1, count=1))
    for dt, pack in ((np.float32, lambda x: x), (np.uint8, ctx.pack_u8), (np.float16, ctx.pack_f16)):
        size = np.dtype(dt).itemsize
        host = rng.integers(0, 256, (h + GUARD, w, 4 * size), dtype=np.uint8).view(dt)
        assert host.shape == (h + GUARD, w, 4)
        got = raw_joint(ctx, fr, gl, HS[:L], 1, 1, 1, win, [host])[0]
        assert same(got[:h], pack(plain)), (cls, shape, np.dtype(dt).name, "the frame's rows")
        assert same(got[h:], host[h:]), (cls, shape, np.dtype(dt).name, "rows beyond the frame")


# ---- 3. every tile count -------------------------------------------------------------------------------------------------------
RAGGED = ((4, 6), (5, 5), (7, 9), (8, 8), (5, 13))          # 24, 25, 63, 64, 65 tiles, the last row and column ragged


def _joint_tile_cases():
    out = []
    for win in ("21x21", "14x14"):
        for T in range(1, 18):                              # a row of T tiles, a column of T tiles
            out += [(win, 2, TILE_H, VW[win] * T), (win, 2, TILE_H * T, VW[win])]
        for L in (2, 3, 4):
            out += [(win, L, TILE_H * ty - 3, VW[win] * tx - 5) for ty, tx in RAGGED]
    return sorted(set(out))


def one_and_two_frames(fr, gl, hs, search, patch):
    """The checker's output of frame 0 alone (k = 0), and output 0 of the two frames at k = 1: np_nlm_joint.nlm_joint's own loop over
    the neighbours, with the pair (0, 0) evaluated once for both."""
    n0, d0 = chk.pair_sums(gl[0], gl[0], fr[0], hs, search, patch)
    n1, d1 = chk.pair_sums(gl[0], gl[1], fr[1], hs, search, patch)
    zn, zd = np.zeros_like(n0), np.zeros_like(d0)
    return chk.normalize(zn + n0, zd + d0), chk.normalize(zn + n0 + n1, zd + d0 + d1)


@pytest.mark.parametrize("win,L,h,w", _joint_tile_cases(), ids=lambda v: str(v))
def test_every_tile_count_of_the_32_row_classes(ctx, win, L, h, w):
    # A tile the remap leaves out keeps the output buffer's old bytes: the outputs are NaN before the call, and every pixel is
    # compared.  A tile dealt twice cannot be seen in one fused output, but in output 0 of two frames at k = 1 each neighbour's
    # sums are added once.  Fresh random data per case.
    search, patch = WIN[win]
    tiles = -(-h // TILE_H) * -(-w // VW[win])
    fr = frames_of((h, w), 2, seed=7919 * h + w + L)
    gl = wrap_guides((h, w), 2, L, seed=31 * h + w + L)
    want1, want2 = one_and_two_frames(fr, gl, HS[:L], search, patch)
    got1 = raw_joint(ctx, fr[:1], gl[:1], HS[:L], 0, 0, 1, win, [nan_frame((h, w))])
    got2 = raw_joint(ctx, fr, gl, HS[:L], 1, 0, 1, win, [nan_frame((h, w))])
    assert not np.isnan(got1[0]).any() and not np.isnan(got2[0]).any(), (win, L, h, w, tiles, "a tile was left out")
    check(f"part 3 {win} L={L} {h}x{w} ({tiles} tiles) one frame", got1, [want1])
    check(f"part 3 {win} L={L} {h}x{w} ({tiles} tiles) two frames", got2, [want2])


@pytest.mark.parametrize("cfg,h,w", _tile_cases(), ids=lambda v: str(v))
def test_every_tile_count_of_the_64_row_class(ctx, cfg, h, w):
    # one layer: the layered filter's tile shape, and by identity 1 its bits -- no checker needed (the layered suite holds that filter
    # against its own at these shapes)
    win = NLM_CFGS[cfg]
    fr = frames_of((h, w), 2, seed=104729 * h + w)
    gl = wrap_guides((h, w), 2, 1, seed=37 * h + w)
    want = ctx.nlm_layers_temporal(fr, gl, 1, 0, 1, hparam=0.37, **win)[0]
    got = raw_joint(ctx, fr, gl, [0.37], 1, 0, 1, (win["search"], win["patch"]), [nan_frame((h, w))])[0]
    assert not np.isnan(got).any() and same(got, want), (cfg, h, w)
    want = ctx.nlm_layers_temporal(fr[:1], gl[:1], 0, hparam=0.37, **win)[0]
    got = raw_joint(ctx, fr[:1], gl[:1], [0.37], 0, 0, 1, (win["search"], win["patch"]), [nan_frame((h, w))])[0]
    assert not np.isnan(got).any() and same(got, want), (cfg, h, w, "one frame")


# ---- 4. HDR colours, the range of h and of h_0 / h_l ----------------------------------------------------------------------------
HDR_SHAPE = (70, 150)
H_SETS = [(0.02, 50.0), (50.0, 0.02), (0.5, 0.5), (2.0, 0.1), (0.1, 2.0), (0.5, 0.02, 50.0, 2.0), (50.0, 50.0, 50.0, 0.02),
          (0.5, 0.02, 50.0, 2.0, 0.3)]


def _hdr(rng, h, w):
    """conftest.synth_hdr with its peak at 6e4: inside binary16, and 441 weights of 1 stay far below fp32 overflow."""
    img = synth_hdr(rng, h, w)
    img[..., :3] *= np.float32(6.0e4) / img[..., :3].max()
    return img.astype(np.float16).astype(np.float32)       # (so that the float16 frames below ARE these frames)


@pytest.mark.parametrize("hs", H_SETS, ids=lambda v: "-".join(f"{x:g}" for x in v))
@pytest.mark.parametrize("win", ["21x21", "14x14"])
def test_hdr_colours_and_the_range_of_h(ctx, win, hs):
    """The header's precision sentence carries no condition on the h or on the colours."""
    search, patch = WIN[win]
    h, w = HDR_SHAPE
    L = len(hs)
    rng = np.random.default_rng(31)
    frames = [_hdr(rng, h, w) for _ in range(2)]
    assert 5.9e4 < max(f.max() for f in frames) < 65504
    gl = wrap_guides(HDR_SHAPE, 2, L, sparse=True)
    # the inputs are not degenerate: the checker's weight sum weighs several offsets, not the centre alone
    den = chk.pair_sums(gl[0], gl[0], frames[0], hs, search, patch)[1] - 0.001
    print(f"part 4 {win} h = {hs}: median weight sum {np.median(den):.1f}")
    assert np.median(den) > 2
    got1 = ctx.nlm_joint(frames[:1], gl[:1], hs, 0, search=search, patch=patch)
    check(f"part 4 {win} h = {hs} HDR one frame", got1, chk.nlm_joint(frames[:1], gl[:1], hs, 0, search, patch))
    got2 = ctx.nlm_joint(frames, gl, hs, 1, search=search, patch=patch)
    check(f"part 4 {win} h = {hs} HDR two frames", got2, chk.nlm_joint(frames, gl, hs, 1, search, patch))
    # the same frames as RGBA16F: the bits of the float32 frames they widen to
    half = [f.astype(np.float16) for f in frames]
    assert all(np.array_equal(a.astype(np.float32), b) for a, b in zip(half, frames))
    assert same(ctx.nlm_joint(half[:1], gl[:1], hs, 0, search=search, patch=patch)[0], got1[0])
    assert all(same(a, b) for a, b in zip(ctx.nlm_joint(half, gl, hs, 1, search=search, patch=patch), got2))


@pytest.mark.parametrize("cls", [(win, L) for win in ("21x21", "14x14") for L in (2, 4, 5)], ids=cls_id)
def test_rgba8_frames_against_the_checker(ctx, cls):
    win, L = cls
    search, patch = WIN[win]
    hs = {2: (2.0, 0.1), 4: H_SETS[5], 5: H_SETS[7]}[L]
    u8 = frames_of(HDR_SHAPE, 2, np.uint8, translucent=True, seed=32 + L)
    gl = wrap_guides(HDR_SHAPE, 2, L, sparse=True)
    check(f"part 4 {win} L={L} h = {hs} RGBA8 two frames", ctx.nlm_joint(u8, gl, hs, 1, search=search, patch=patch),
          chk.nlm_joint(u8, gl, hs, 1, search, patch))


# ---- 5. non-finite texels, in opaque and in general tiles ------------------------------------------------------------------------
NF_HS = (0.05, 0.03, 0.05, 0.04, 0.05)


def step_guides(L):
    """Guides of 0 and 255 only: a step in x at column 95, a step in y at row 70, and so on in turn.  With h <= 0.05 one mismatching
    texel gives at most exp(-1200), 0 in fp32 and in float64: every weight is exactly 0 or 1 on both sides, no flushed tiny weight
    separates Inf * 0 = NaN from Inf * tiny = Inf, and the h are unequal, so r_l != 1."""
    gx = np.full(BIG + (4,), 255, np.uint8)
    gx[:, :95, :3] = 0
    gy = np.full(BIG + (4,), 255, np.uint8)
    gy[:70, :, :3] = 0
    return [[(gx, gy)[l % 2].copy() for l in range(L)] for _ in range(2)]


def non_finite_frames(which):
    """Frame 0 clean, the odd texels in frame 1 only (rounded through binary16, so that the float16 frames ARE these frames)."""
    fr = [f.astype(np.float16).astype(np.float32) for f in frames_of(BIG, 2, seed=80)]
    if which == "mixed":
        fr[1][1, 2, :3] = np.inf            # near a frame corner (alpha stays 1): a border tile, the general form
        fr[1][60, 94] = -np.inf             # beside the x step, all four channels
        fr[1][66, 100, 1] = np.nan          # in the second tile row and column of every class
        fr[1][100, 120, 3] = np.nan         # in alpha alone: no colour channel may turn NaN with it
    else:
        assert (fr[1][..., 3] == 1).all()
        fr[1][ODD][:3] = np.inf             # alpha 1 everywhere: the interior tiles take 0.001 + acc.w with a non-finite colour sum
    return fr


@pytest.mark.parametrize("which", ["mixed", "opaque"])
@pytest.mark.parametrize("cls", STRIP + [("21x21", 5)], ids=cls_id)
def test_non_finite_texels_propagate_like_the_checker(ctx, cls, which):
    win, L = cls
    search, patch = WIN[win]
    hs = NF_HS[:L]
    assert L == 1 or len(set(hs)) > 1
    fr, gl = non_finite_frames(which), step_guides(L)
    with np.errstate(all="ignore"):
        want = chk.nlm_joint(fr, gl, hs, 1, search, patch)
    for t in range(2):                      # both outputs owe their odd values to frame 1
        if which == "mixed":
            assert np.isnan(want[t]).any() and np.isposinf(want[t]).any() and np.isneginf(want[t]).any(), (cls, t)
        assert not np.isfinite(want[t]).all() and np.isfinite(want[t]).any(), (cls, t)
    assert np.isfinite(chk.nlm_joint(fr[:1], gl[:1], hs, 0, search, patch)[0]).all()
    got = ctx.nlm_joint(fr, gl, hs, 1, search=search, patch=patch)
    e = max(same_masks_and_values(got[t], want[t], (cls, which, "output", t)) for t in range(2))
    if L == 1:                              # identity 1
        lay = ctx.nlm_layers_temporal(fr, gl, 1, hparam=hs[0], search=search, patch=patch)
        assert all(same(a, b) for a, b in zip(got, lay)), (cls, which)
    if which == "mixed":                    # the same texels as RGBA16F frames
        half = [f.astype(np.float16) for f in fr]
        assert all(np.array_equal(bits(a.astype(np.float32)), bits(b)) for a, b in zip(half, fr))
        got16 = ctx.nlm_joint(half, gl, hs, 1, search=search, patch=patch)
        for t in range(2):
            same_masks_and_values(got16[t], want[t], (cls, which, "float16 frames, output", t))
    print(f"part 5 {win} L={L} {which}: finite values {e:.2e}; output 0: {int(np.isnan(want[0]).sum())} NaN, {int(np.isposinf(want[0]).sum())} +Inf, "
          f"{int(np.isneginf(want[0]).sum())} -Inf, {int(np.isfinite(want[0]).sum())} finite")


# ---- 6. what the call must not read --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [("21x21", 1), ("21x21", 2), ("21x21", 4), ("7x7", 2)], ids=cls_id)
def test_the_guides_alpha_byte_is_not_read(ctx, cls):
    win, L = cls
    search, patch = WIN[win]
    rng = np.random.default_rng(51)
    fr = frames_of(HDR_SHAPE, 2, translucent=True, seed=52)
    gl = wrap_guides(HDR_SHAPE, 2, L)
    other = [[g.copy() for g in ls] for ls in gl]
    for ls in other:
        for g in ls:
            g[..., 3] = rng.integers(0, 255, HDR_SHAPE)         # (never the 255 the guides carry)
    assert all((a[..., 3] != b[..., 3]).all() and np.array_equal(a[..., :3], b[..., :3]) for x, y in zip(gl, other) for a, b in zip(x, y))
    got = ctx.nlm_joint(fr, gl, HS[:L], 1, search=search, patch=patch)
    check(f"part 6 alpha {win} L={L}", got, chk.nlm_joint(fr, gl, HS[:L], 1, search, patch))
    assert all(same(a, b) for a, b in zip(ctx.nlm_joint(fr, other, HS[:L], 1, search=search, patch=patch), got)), cls


@pytest.mark.parametrize("cls", [("21x21", 2), ("7x7", 2)], ids=cls_id)
def test_frames_outside_the_window_are_not_read(ctx, cls):
    """first = 1, count = 1, k = 1 on four frames reads the frames and layers of [0, 3): frame 3 and its layers are valid buffers of
    NaN colours and random guide bytes, and the output is the output of the three-frame sequence."""
    win, L = cls
    search, patch = WIN[win]
    rng = np.random.default_rng(61)
    fr = frames_of(HDR_SHAPE, 3, translucent=True, seed=62)
    gl = wrap_guides(HDR_SHAPE, 3, L)
    want = ctx.nlm_joint(fr, gl, HS[:L], 1, first=1, count=1, search=search, patch=patch)
    check(f"part 6 window {win} L={L}", want, chk.nlm_joint(fr, gl, HS[:L], 1, search, patch, first=1, count=1))
    fr4 = fr + [nan_frame(HDR_SHAPE)]
    gl4 = gl + [[rng.integers(0, 256, HDR_SHAPE + (4,), dtype=np.uint8) for _ in range(L)]]
    got = ctx.nlm_joint(fr4, gl4, HS[:L], 1, first=1, count=1, search=search, patch=patch)
    assert len(got) == 1 and same(got[0], want[0]), cls
    # ... and frame 0 likewise when the window starts behind it: first = 2, k = 1 reads [1, 4)
    fr0 = [nan_frame(HDR_SHAPE)] + fr
    gl0 = gl4[3:] + gl
    got = ctx.nlm_joint(fr0, gl0, HS[:L], 1, first=2, count=1, search=search, patch=patch)
    assert len(got) == 1 and same(got[0], want[0]), (cls, "a frame before the window")
