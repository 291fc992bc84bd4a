"""GPU suite: what the a-trous filters (include/mi_denoise.h, sections a4g and a4h) touch beside their buffers, strip-shaped
frames, and sub-ranges of the temporal call.

    * Guard bands.  Through the raw C calls, the output(s) and the scratch sit in the middle of larger device allocations with a
      4096-byte band of sentinel bytes on either side; the scratch is exactly mid_atrous_scratch_bytes long, so with two passes
      the band begins where the first level ends.  After the call every band, every frame and every layer has its bytes, and the
      outputs have the bits of the plain ctx call.
    * Poisoned surroundings.  Frames and layers sit in allocations whose other bytes are 0xff (NaN as float32 and as float16): a
      tap read outside the image but inside the allocation must not reach the sums even with weight 0 (NaN * 0 = NaN).
    * Strips of 262 149 x 2 and 2 x 262 149 texels (the two global-tap kernels launch a two-dimensional grid: 65 538 workgroups
      in y for the tall one) and of 1 x 70 000 and 70 000 x 1, against the float64 checkers.
    * Sub-ranges.  Output t of mid_atrous_joint_temporal over [first, first + count) has the bits of output t of the whole call, and
      is within 1e-5 max(1, |ref|) of the float64 checker.
"""
import ctypes

import numpy as np
import pytest

import guide_format_inputs as gi
import image_denoising_filter_amd as mid
import np_atrous_joint as chk
import np_atrous_temporal as chk_t
from conftest import rel_err

pytestmark = pytest.mark.gpu

BAND = 4096
SHAPES = [(33, 130), (21, 70)]
LAYERS = (1, 3, 4, 5)
ODT = (np.float32, np.float16, np.uint8)
SIGMAS = (1.0, 2.0, 0.5)
TOL = 1e-5
FMT = {np.dtype(np.float32): mid.FMT_RGBA32F, np.dtype(np.float16): mid.FMT_RGBA16F, np.dtype(np.uint8): mid.FMT_RGBA8}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Banded:
    """`nbytes` of device memory with BAND bytes before and after it in the same allocation.  payload: the bytes of the middle (an
    array), else the middle holds sentinel bytes too; fill: the byte of the surroundings, None = pseudo-random sentinel bytes."""

    def __init__(self, ctx, nbytes, payload=None, fill=None, seed=0):
        self.ctx, self.nbytes = ctx, int(nbytes)
        if fill is None:
            self.host = np.random.default_rng(seed).integers(0, 256, self.nbytes + 2 * BAND, dtype=np.uint8)
        else:
            self.host = np.full(self.nbytes + 2 * BAND, fill, np.uint8)
        if payload is not None:
            raw = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
            assert raw.size == self.nbytes
            self.host[BAND:BAND + self.nbytes] = raw
        self.buf = ctx.upload(self.host)
        self.ptr = self.buf.ptr + BAND

    def read(self):
        return self.ctx.download(self.buf, self.host.shape, np.uint8)

    def bands_intact(self):
        now = self.read()
        return np.array_equal(now[:BAND], self.host[:BAND]) and np.array_equal(now[BAND + self.nbytes:], self.host[BAND + self.nbytes:])

    def unchanged(self):
        return np.array_equal(self.read(), self.host)

    def middle(self, shape, dtype):
        return self.read()[BAND:BAND + self.nbytes].view(dtype).reshape(shape)


def frames_of(shape, n, odt):
    fr = gi.hdr_frames(shape, n, seed=11)
    return [np.clip(f / 4, 0, 1).astype(np.float32) for f in fr] if odt == np.uint8 else fr


def layers_of(shape, n, dt, L):
    sets = [gi.render_layers(shape, n, dt, seed=12 + s) for s in range((L + 2) // 3)]
    return [[sets[l // 3][f][l % 3] for l in range(L)] for f in range(n)]


def sigmas_of(L):
    return [SIGMAS[l % 3] for l in range(L)]


def raw_single(ctx, fr, ly, sg, passes, cs, odt, fill):
    """mid_atrous_joint with every buffer inside a larger allocation; asserts bands and inputs, returns the output."""
    h, w = fr.shape[:2]
    L = len(ly)
    d_in = Banded(ctx, fr.nbytes, fr, fill, seed=1)
    d_l = [Banded(ctx, l.nbytes, l, fill, seed=2 + i) for i, l in enumerate(ly)]
    p = mid.AtrousParams(w, h, 0, passes, cs, mid.api.fmt_with_guide(FMT[fr.dtype], FMT[ly[0].dtype]))
    d_out = Banded(ctx, h * w * 4 * np.dtype(odt).itemsize, seed=40)
    nscr = mid.lib.mid_atrous_scratch_bytes(ctypes.byref(p))
    assert nscr == (0, 0, 1, 2, 2, 2, 2, 2, 2)[passes] * h * w * 16
    d_scr = Banded(ctx, nscr, seed=41) if nscr else None
    rc = mid.lib.mid_atrous_joint(ctx.handle, ctypes.byref(p), (ctypes.c_float * 16)(*sg), d_in.ptr, (ctypes.c_void_p * 17)(*[d.ptr for d in d_l]), L,
                                  d_out.ptr, FMT[np.dtype(odt)], d_scr.ptr if d_scr else None, None)
    assert rc == 0, mid.lib.mid_last_error()
    ctx.sync()
    assert d_out.bands_intact(), "a store beside out"
    assert d_scr is None or d_scr.bands_intact(), "a store beside the scratch levels"
    assert d_in.unchanged() and all(d.unchanged() for d in d_l), "an input changed"
    return d_out.middle((h, w, 4), odt)


def raw_temporal(ctx, frames, layers, sg, k, first, count, passes, cs, odt, fill):
    h, w = frames[0].shape[:2]
    n, L = len(frames), len(layers[0])
    d_fr = [Banded(ctx, f.nbytes, f, fill, seed=1 + i) for i, f in enumerate(frames)]
    d_l = [Banded(ctx, l.nbytes, l, fill, seed=20 + i) for i, l in enumerate(l for ls in layers for l in ls)]
    p = mid.AtrousParams(w, h, 0, passes, cs, mid.api.fmt_with_guide(FMT[frames[0].dtype], FMT[layers[0][0].dtype]))
    d_out = [Banded(ctx, h * w * 4 * np.dtype(odt).itemsize, seed=200 + i) for i in range(count)]
    nscr = mid.lib.mid_atrous_scratch_bytes(ctypes.byref(p))
    d_scr = Banded(ctx, nscr, seed=300) if nscr else None
    rc = mid.lib.mid_atrous_joint_temporal(ctx.handle, ctypes.byref(p), (ctypes.c_float * 16)(*sg), (ctypes.c_void_p * n)(*[d.ptr for d in d_fr]),
                                           (ctypes.c_void_p * len(d_l))(*[d.ptr for d in d_l]), L, n, k, first, count,
                                           (ctypes.c_void_p * count)(*[d.ptr for d in d_out]), FMT[np.dtype(odt)], d_scr.ptr if d_scr else None, None)
    assert rc == 0, mid.lib.mid_last_error()
    ctx.sync()
    assert all(d.bands_intact() for d in d_out), "a store beside an output"
    assert d_scr is None or d_scr.bands_intact(), "a store beside the scratch levels"
    assert all(d.unchanged() for d in d_fr) and all(d.unchanged() for d in d_l), "an input changed"
    return [d.middle((h, w, 4), odt) for d in d_out]


# ---- 1. guard bands --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bands_single_frame(ctx, shape, L):
    n = 0
    for pi, passes in enumerate((1, 2, 3, 8)):
        for oi, odt in enumerate(ODT):
            gdt = (np.float32, np.float16)[(pi + oi + L) % 2]
            cs = (0.0, 1.0)[(pi + oi) % 2]
            fr, ly, sg = frames_of(shape, 1, odt)[0], layers_of(shape, 1, gdt, L)[0], sigmas_of(L)
            got = raw_single(ctx, fr, ly, sg, passes, cs, odt, None)
            want = ctx.atrous_joint(fr, ly, sg, passes=passes, color_sigma=cs, out_dtype=odt)
            assert same(got, want), (shape, L, passes, np.dtype(odt).name)
            n += 1
    assert n == 12


@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bands_temporal(ctx, shape, L):
    for pi, passes in enumerate((1, 2, 3, 8)):
        odt = ODT[(pi + L) % 3]
        gdt = (np.float32, np.float16)[(pi + L) % 2]
        cs = (0.0, 1.0)[pi % 2]
        fr, ly, sg = frames_of(shape, 4, odt), layers_of(shape, 4, gdt, L), sigmas_of(L)
        got = raw_temporal(ctx, fr, ly, sg, 2, 1, 2, passes, cs, odt, None)
        want = ctx.atrous_joint_temporal(fr, ly, sg, k=2, first=1, count=2, passes=passes, color_sigma=cs, out_dtype=odt)
        assert len(got) == 2 and all(same(g, w) for g, w in zip(got, want)), (shape, L, passes, np.dtype(odt).name)


# ---- 2. poisoned surroundings ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nan_around_frames_and_layers(ctx, shape, L):
    assert np.isnan(np.full(4, 0xff, np.uint8).view(np.float32)).all() and np.isnan(np.full(2, 0xff, np.uint8).view(np.float16)).all()
    for dt in (np.float32, np.float16):
        cs = 1.0 if dt == np.float32 else 0.0
        fr = [f.astype(dt) for f in gi.hdr_frames(shape, 4, seed=11)]
        ly, sg = layers_of(shape, 4, dt, L), sigmas_of(L)
        got = raw_single(ctx, fr[0], ly[0], sg, 3, cs, np.float32, 0xff)
        assert not np.isnan(got).any()
        assert same(got, ctx.atrous_joint(fr[0], ly[0], sg, passes=3, color_sigma=cs)), (shape, L, np.dtype(dt).name)
        got = raw_temporal(ctx, fr, ly, sg, 2, 1, 2, 3, cs, np.float32, 0xff)
        want = ctx.atrous_joint_temporal(fr, ly, sg, k=2, first=1, count=2, passes=3, color_sigma=cs)
        for g, w in zip(got, want):
            assert not np.isnan(g).any()
            assert same(g, w), (shape, L, np.dtype(dt).name, "temporal")


# ---- 3. strips -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 5])
@pytest.mark.parametrize("shape", [(262149, 2), (2, 262149)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_long_strips(ctx, shape, L):
    fr = gi.hdr_frames(shape, 1, seed=11)[0]
    ly, sg = layers_of(shape, 1, np.float32, L)[0], sigmas_of(L)
    got = ctx.atrous_joint(fr, ly, sg, passes=2, color_sigma=1.0)
    err = rel_err(got, chk.atrous_joint(fr, ly, sg, passes=2, color_sigma=1.0))
    print(f"{shape} L={L}, 2 passes: {err:.3e}")
    assert np.isfinite(got).all() and err <= TOL, (shape, L, err)


def test_long_strip_temporal(ctx):
    shape, L = (262149, 2), 5
    fr, ly, sg = gi.hdr_frames(shape, 3, seed=11), layers_of(shape, 3, np.float32, L), sigmas_of(L)
    # the middle output: the one whose window holds all three frames (the float64 checker of all three outputs takes 10 s)
    (got,) = ctx.atrous_joint_temporal(fr, ly, sg, k=1, first=1, count=1, passes=1, color_sigma=1.0)
    (ref,) = chk_t.atrous_joint_temporal(fr, ly, sg, 1, passes=1, color_sigma=1.0, first=1, count=1)
    err = rel_err(got, ref)
    print(f"{shape} L={L} temporal k=1 t=1: {err:.3e}")
    assert np.isfinite(got).all() and err <= TOL, err


@pytest.mark.parametrize("shape", [(1, 70000), (70000, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_texel_wide_strips_through_eight_passes(ctx, shape):
    L = 4
    fr = gi.hdr_frames(shape, 1, seed=11)[0]
    ly, sg = layers_of(shape, 1, np.float16, L)[0], sigmas_of(L)
    got = ctx.atrous_joint(fr, ly, sg, passes=8, color_sigma=4.0)
    err = rel_err(got, chk.atrous_joint(fr, ly, sg, passes=8, color_sigma=4.0))
    print(f"{shape} L={L}, 8 passes: {err:.3e}")
    assert np.isfinite(got).all() and err <= TOL, (shape, err)


# ---- 4. sub-ranges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [3, 5])
def test_sub_ranges_are_the_whole_call_and_the_checker(ctx, L):
    shape, n, k = (21, 70), 6, 2
    fr, ly, sg = gi.hdr_frames(shape, n, seed=11), layers_of(shape, n, np.float32, L), sigmas_of(L)
    whole = ctx.atrous_joint_temporal(fr, ly, sg, k=k, passes=3, color_sigma=1.0)
    assert len(whole) == n
    for first, count in ((0, 1), (2, 3), (5, 1)):
        got = ctx.atrous_joint_temporal(fr, ly, sg, k=k, first=first, count=count, passes=3, color_sigma=1.0)
        ref = chk_t.atrous_joint_temporal(fr, ly, sg, k, passes=3, color_sigma=1.0, first=first, count=count)
        assert len(got) == count == len(ref)
        for i in range(count):
            assert same(got[i], whole[first + i]), (L, first, count, i)
            err = rel_err(got[i], ref[i])
            print(f"L={L} first={first} count={count} t={first + i}: {err:.3e}")
            assert err <= TOL, (L, first, count, i, err)
