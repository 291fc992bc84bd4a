"""GPU suite: mid_firefly_clamp (include/mi_denoise.h, section a4l) against tests/np_firefly.py, BIT FOR BIT.

Through the raw C call, every buffer in the middle of a larger device allocation: the output holds NaN before the call and sits
between two 4096-byte guard bands that must keep their bytes; the input must keep its own.  Frame formats u8 / f16 / f32; the
frames are tests/firefly_inputs.py's (fireflies of 4096 x, NaN, +-Inf and negative channels), which tests/test_firefly_args.py
holds to their conditions with the checker alone.  Shapes from 1 x 1 to 67 x 131, one past both tile seams (17 x 65), every height
1..34 at width 70, columns of one pixel beyond the launch's tile cap, a 262149 x 2 strip; every (radius, rank) and both
(gain, floor) pairs inside each.

"Bit for bit" leaves out what IEEE 754 leaves open: where the checker has a NaN the kernel must have a NaN, of any sign and
payload.  Every other value has the checker's bits.
"""
import ctypes

import numpy as np
import pytest
import torch

import image_denoising_filter_amd as mid
import np_firefly as chk
from firefly_inputs import GAIN_FLOOR, PARAMS, frame_of, plant
from np_albedo import widen
from test_gpu_albedo import same_but_nan
from test_gpu_atrous_bounds import FMT, Banded, bits

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (2, 1), (3, 3), (1, 63), (16, 64), (17, 65), (65, 1), (33, 129), (67, 131)]          # (h, w)
DTYPES = (np.uint8, np.float16, np.float32)
IDS = dict(ids=lambda d: np.dtype(d).name)


def raw_clamp(ctx, fr, radius=1, rank=1, gain=1.0, floor=0.0):
    h, w = fr.shape[:2]
    d_in = Banded(ctx, fr.nbytes, fr, seed=1)
    d_out = Banded(ctx, h * w * 16, fill=0xff)
    p = mid.FireflyParams(w, h, radius, rank, gain, floor, FMT[fr.dtype])
    rc = mid.lib.mid_firefly_clamp(ctx.handle, ctypes.byref(p), d_in.ptr, d_out.ptr, None)
    assert rc == 0, mid.lib.mid_last_error()
    ctx.sync()
    assert d_out.bands_intact(), "a store beside out"
    assert d_in.unchanged(), "the input changed"
    return d_out.middle((h, w, 4), np.float32)


def every_setting(ctx, fr, note):
    for radius, rank in PARAMS:
        for gain, floor in GAIN_FLOOR:
            got = raw_clamp(ctx, fr, radius, rank, gain, floor)
            assert same_but_nan(got, chk.firefly_clamp(fr, radius, rank, gain, floor)), (note, radius, rank, gain, floor)
            assert np.array_equal(bits(got[..., 3]), bits(widen(fr)[..., 3])), "alpha passes through, bit for bit"


@pytest.mark.parametrize("dt", DTYPES, **IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_clamp_has_the_checker_bits(ctx, shape, dt):
    every_setting(ctx, frame_of(shape, dt, shape[0] + shape[1]), shape)


@pytest.mark.parametrize("dt", (np.float16, np.float32), **IDS)
def test_every_height_at_width_70(ctx, dt):
    for h in range(1, 35):
        fr = frame_of((h, 70), dt, 100 + h)
        radius, rank = PARAMS[h % len(PARAMS)]
        for r2, k2 in ((radius, rank), (3 - radius, 5 - rank)):
            got = raw_clamp(ctx, fr, r2, k2, 1.0, 0.0)
            assert same_but_nan(got, chk.firefly_clamp(fr, r2, k2, 1.0, 0.0)), (h, r2, k2)


@pytest.mark.parametrize("dt", (np.float16, np.float32), **IDS)
def test_planted_on_corners_edges_and_tile_seams(ctx, dt):
    h, w = 35, 131
    base = frame_of((h, w), dt, 7)
    corners = plant(base, (0, h - 1), (0, w - 1))
    edges = plant(base, (0, h - 1), range(1, w - 1, 3))
    edges = plant(edges, range(1, h - 1, 3), (0, w - 1), values=(np.inf, 4096.0, -np.inf, np.nan))
    seams = plant(base, range(h), (63, 64), values=(4096.0, np.nan, 4096.0, np.inf, -np.inf))
    seams = plant(seams, (15, 16), range(0, w, 2), values=(np.nan, 4096.0, np.inf, 4096.0, -np.inf))
    for name, fr in (("corners", corners), ("edges", edges), ("seams", seams)):
        assert np.isnan(fr).any() and np.isinf(fr).any(), name
        every_setting(ctx, fr, name)


def test_strips_beyond_the_tile_cap(ctx):
    """The launch deals its tiles to at most 8 workgroups per CU, which then stride: a 262149 x 2 strip has 4097 tiles, a column of
    one pixel and 40000 rows 2500."""
    cap = torch.cuda.get_device_properties(0).multi_processor_count * 8
    for shape, dt, radius, rank in (((2, 262149), np.float32, 2, 2), ((2, 262149), np.uint8, 1, 1), ((40000, 1), np.float16, 2, 3)):
        assert -(-shape[0] // 16) * -(-shape[1] // 64) > cap, "the tile cap is not passed"
        fr = frame_of(shape, dt, 9)
        got = raw_clamp(ctx, fr, radius, rank, 1.0, 0.0)
        assert same_but_nan(got, chk.firefly_clamp(fr, radius, rank, 1.0, 0.0)), shape


C0 = np.float32([0.375, 0.5, 0.25, 0.75])


@pytest.mark.parametrize("dt", (np.float16, np.float32), **IDS)
def test_the_4096_identity(ctx, dt):
    h, w = 35, 131
    clean = np.broadcast_to(C0, (h, w, 4)).astype(dt)
    one = clean.copy()
    for y, x in ((0, 0), (h - 1, w - 1), (15, 63), (20, 64), (16, 100)):              # more than two pixels apart: no one's neighbour at radius 2
        one[y, x, :3] *= dt(4096)
    for radius in (1, 2):
        assert np.array_equal(bits(raw_clamp(ctx, one, radius, 1)), bits(clean.astype(np.float32))), radius
    pair = clean.copy()
    pair[15:17, 63, :3] *= dt(4096)                                                    # a pair across the horizontal seam
    pair[30, 64:66, :3] *= dt(4096)
    assert np.array_equal(bits(raw_clamp(ctx, pair, 1, 1)), bits(pair.astype(np.float32))), "each is the other's maximum"
    assert np.array_equal(bits(raw_clamp(ctx, pair, 1, 2)), bits(clean.astype(np.float32)))
    block = clean.copy()
    block[15:17, 63:65, :3] *= dt(4096)                                                # a 2 x 2 block on the corner of four tiles
    assert np.array_equal(bits(raw_clamp(ctx, block, 2, 3)), bits(block.astype(np.float32)))
    assert np.array_equal(bits(raw_clamp(ctx, block, 2, 4)), bits(clean.astype(np.float32)))


def test_the_python_method(ctx):
    for dt in DTYPES:
        fr = frame_of((33, 129), dt, 3)
        assert same_but_nan(ctx.firefly_clamp(fr), chk.firefly_clamp(fr))
        assert same_but_nan(ctx.firefly_clamp(fr, radius=2, rank=3, gain=1.5, floor=0.25), chk.firefly_clamp(fr, 2, 3, 1.5, 0.25))


def test_refusals_leave_the_output_untouched(ctx):
    h, w = 9, 33
    fr = frame_of((h, w), np.float32, 60)
    d_in, d_out = Banded(ctx, fr.nbytes, fr, seed=5), Banded(ctx, h * w * 16, seed=7)

    def refused(needle, width=w, height=h, radius=1, rank=1, gain=1.0, floor=0.0, fmt=mid.FMT_RGBA32F, pin=d_in.ptr, pout=d_out.ptr, params=True):
        p = mid.FireflyParams(width, height, radius, rank, gain, floor, fmt)
        rc = mid.lib.mid_firefly_clamp(ctx.handle, ctypes.byref(p) if params else None, pin, pout, None)
        msg = mid.lib.mid_last_error().decode()
        assert rc == 1 and needle in msg, (rc, msg)
        ctx.sync()
        assert d_out.unchanged() and d_in.unchanged(), "a refused call wrote"

    refused("params is NULL", params=False)
    refused("NULL pointer", pin=None)
    refused("NULL pointer", pout=None)
    for bad in (0, 3, -1):
        refused("radius", radius=bad)
    for bad in (0, 5, -1):
        refused("rank", rank=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        refused("gain", gain=bad)
    for bad in (-1e-3, float("nan"), float("inf")):
        refused("floor", floor=bad)
    refused("bad size", width=0)
    refused("bad size", height=-1)
    refused("too large", width=1 << 15, height=1 << 15)
    refused("unknown format", fmt=3)
    refused("guide bits", fmt=mid.api.fmt_with_guide(mid.FMT_RGBA32F, mid.FMT_RGBA32F))
    refused("guide bits", fmt=mid.FMT_RGBA8 | (1 << 8))
    refused("in is not 16-byte aligned", pin=d_in.ptr + 4)
    refused("in is not 8-byte aligned", fmt=mid.FMT_RGBA16F, pin=d_in.ptr + 4)
    refused("in is not 4-byte aligned", fmt=mid.FMT_RGBA8, pin=d_in.ptr + 2)
    refused("out is not 16-byte aligned", pout=d_out.ptr + 8)
    refused("out overlaps in", pout=d_in.ptr)                                          # exactly in place: a stencil cannot
    refused("out overlaps in", pout=d_in.ptr + 16)
    refused("out overlaps in", pout=d_in.ptr - 16)
    refused("out overlaps in", pout=d_in.ptr + 16 * (h * w - 1))
    refused("out overlaps in", fmt=mid.FMT_RGBA8, pout=d_in.ptr)
    refused("out overlaps in", fmt=mid.FMT_RGBA16F, pin=d_out.ptr + 16 * h * w - 8)    # the last input texel inside out
