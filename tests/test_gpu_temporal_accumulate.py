"""GPU suite: the recursive temporal accumulation (mid_temporal_accumulate, include/mi_denoise.h section a4j) against its float64
checker (tests/np_temporal_accumulate.py), and the bit identities the header states.

Tolerances, the header's: colour, m1, m2 within 1e-5 max(1, |ref|); N' within 1e-5 max(1, N'); the variance within
1e-5 max(1, m2_ref) -- both terms of v = m2' - m1'^2 carry the rounding of a value of m2's size.  The inputs
(tests/temporal_accumulate_inputs.py) reject part of the history, believe part of it and half believe the rest:
tests/test_temporal_accumulate_args.py holds them to that on the CPU.
"""
import numpy as np
import pytest

import temporal_accumulate_inputs as tai
from np_temporal_accumulate import temporal_accumulate as check
from test_gpu_atrous_bounds import same

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 63), (4, 64), (9, 65), (131, 261)]       # (h, w): 1 x 1, 63 x 5, 64 x 4, 65 x 9, 261 x 131
LAYERS = (0, 1, 3, 5, 16)
DT = (np.float32, np.float16, np.uint8)
TOL = 1e-5


def errors(got, ref):
    col, st, var = (a.astype(np.float64) for a in got)
    rs = ref["state"]

    def rel(a, b, scale):
        with np.errstate(invalid="ignore"):
            e = np.abs(a - b) / np.maximum(1.0, scale)
        assert np.array_equal(np.isnan(a), np.isnan(b))
        return float(np.nanmax(e)) if e.size else 0.0
    e = {"colour": rel(col, ref["colour"], np.abs(ref["colour"])), "moments": rel(st[..., :2], rs[..., :2], np.abs(rs[..., :2])),
         "N": rel(st[..., 2], rs[..., 2], rs[..., 2]), "variance": rel(var, ref["variance"], rs[..., 1])}
    assert not st[..., 3].any()
    return e


def case(shape, L, fdt, gdt, motion, with_var, setting, t=1, hist="random"):
    kw = dict(hist=tai.history_of(shape) if hist == "random" else hist, motion=tai.motion_of(shape, motion),
              var_spatial=tai.var_spatial_of(shape) if with_var else None, **tai.SETTINGS[setting])
    return (tai.frame_of(shape, t, fdt), tai.layers_of(shape, L, gdt, t), tai.layers_of(shape, L, gdt, t - 1), tai.sigmas_of(L)), kw


@pytest.mark.parametrize("L", LAYERS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_against_the_float64_checker(ctx, shape, L):
    # every motion field per (shape, L); frame and guide dtypes, var_spatial and the two settings rotate so that each value
    # meets each (shape, L) class several times over the table
    base = SHAPES.index(shape) + LAYERS.index(L)
    for mi, motion in enumerate(tai.MOTIONS):
        fdt, gdt = DT[(base + mi) % 3], DT[(base + 2 * mi + 1) % 3]
        with_var, setting = (base + mi) % 2 == 0, (base + mi // 2) % 2
        args, kw = case(shape, L, fdt, gdt, motion, with_var, setting)
        e = errors(ctx.temporal_accumulate(*args, **kw), check(*args, **kw))
        print(f"{shape[1]}x{shape[0]} L={L} {np.dtype(fdt).name}/{np.dtype(gdt).name} motion {motion} var_spatial {with_var} setting {setting}: "
              + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert max(e.values()) <= TOL, e


@pytest.mark.parametrize("fdt", DT, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("gdt", DT, ids=lambda d: np.dtype(d).name)
def test_every_format_pair_with_every_motion(ctx, fdt, gdt):
    for mi, motion in enumerate(tai.MOTIONS):
        for with_var in (False, True):
            args, kw = case((9, 65), 3, fdt, gdt, motion, with_var, mi % 2)
            e = errors(ctx.temporal_accumulate(*args, **kw), check(*args, **kw))
            assert max(e.values()) <= TOL, (motion, with_var, e)


@pytest.mark.parametrize("setting", (0, 1))
def test_a_chain_of_six_frames_step_by_step(ctx, setting):
    # every step's checker input is the GPU's own previous state: the tolerance stays a one-step tolerance
    shape, L = (131, 261), 3
    hist = None
    lengths = []
    for t in range(6):
        args, kw = case(shape, L, np.float32, np.uint8, "smooth", True, setting, t=t + 1, hist=hist)
        got = ctx.temporal_accumulate(*args, **kw)
        e = errors(got, check(*args, **kw))
        print(f"chain step {t} setting {setting}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert max(e.values()) <= TOL, (t, e)
        hist = (got[0], got[1])
        lengths.append(float(got[1][..., 2].max()))
    assert lengths[0] == 1.0 and lengths[-1] > 3.0, lengths                                     # the history grows somewhere ...
    assert (hist[1][..., 2] == 1.0).any()                                                       # ... and is rejected somewhere


# ---- bit identities -----------------------------------------------------------------------------------------------------------

def widened(frame):
    return frame.astype(np.float32) / np.float32(255) if frame.dtype == np.uint8 else frame.astype(np.float32)


@pytest.mark.parametrize("fdt", DT, ids=lambda d: np.dtype(d).name)
def test_no_history_gives_the_frame_and_the_spatial_variance(ctx, fdt):
    shape = (9, 65)
    for L in (0, 3):
        (fr, ly, pl, sg), kw = case(shape, L, fdt, np.uint8, "smooth", True, 0, hist=None)
        col, st, var = ctx.temporal_accumulate(fr, ly, pl, sg, **kw)
        assert same(col, widened(fr))
        l = st[..., 0]
        assert same(st[..., 1], l * l) and np.all(st[..., 2] == 1.0) and not st[..., 3].any()
        assert same(var, kw["var_spatial"])
        ref = check(fr, ly, pl, sg, **kw)
        assert np.max(np.abs(l - ref["state"][..., 0])) <= TOL * max(1.0, ref["state"][..., 0].max())


def test_no_motion_plane_is_an_all_zero_motion_plane(ctx):
    for shape, L in (((9, 65), 3), ((131, 261), 5)):
        args, kw = case(shape, L, np.float32, np.float16, "none", True, 0)
        a = ctx.temporal_accumulate(*args, **kw)
        for zero in (0.0, -0.0):
            kw["motion"] = np.full(shape + (2,), zero, np.float32)
            b = ctx.temporal_accumulate(*args, **kw)
            assert all(same(x, y) for x, y in zip(a, b)), (shape, L, zero)


def test_integer_motion_is_the_zero_motion_call_on_the_shifted_history(ctx):
    # equal layers in both frames (every weight 1 or, between different texels, whatever the layers say -- so the PREVIOUS layers are
    # shifted with the history): pixel p with motion (dx, dy) reads texel p + (dx, dy), which the shifted planes hold at p
    shape, L = (131, 261), 3
    h, w = shape
    for dx, dy in ((3, -2), (-5, 4), (0, 1)):
        (fr, ly, pl, sg), kw = case(shape, L, np.float32, np.uint8, "none", True, 0)
        kw["motion"] = np.broadcast_to(np.float32([dx, dy]), shape + (2,)).copy()
        moved = ctx.temporal_accumulate(fr, ly, pl, sg, **kw)
        shift = lambda a: np.roll(a, (-dy, -dx), (0, 1))
        kw["motion"] = None
        kw["hist"] = tuple(shift(a) for a in kw["hist"])
        still = ctx.temporal_accumulate(fr, ly, [shift(a) for a in pl], sg, **kw)
        yy, xx = np.mgrid[0:h, 0:w]
        inside = (xx + dx >= 0) & (xx + dx < w) & (yy + dy >= 0) & (yy + dy < h)
        assert inside.mean() > 0.9
        assert all(same(x[inside], y[inside]) for x, y in zip(moved, still)), (dx, dy)


def test_packed_frames_and_guides_are_the_float_ones_they_widen_to(ctx):
    shape, L = (9, 65), 3
    for dt in (np.uint8, np.float16):
        (fr, ly, pl, sg), kw = case(shape, L, dt, dt, "smooth", True, 1)
        a = ctx.temporal_accumulate(fr, ly, pl, sg, **kw)
        b = ctx.temporal_accumulate(widened(fr), ly, pl, sg, **kw)                              # the frame alone
        assert all(same(x, y) for x, y in zip(a, b)), np.dtype(dt).name
        c = ctx.temporal_accumulate(fr, [widened(g) for g in ly], [widened(g) for g in pl], sg, **kw)     # a4g's guide identity
        assert all(same(x, y) for x, y in zip(a, c)), np.dtype(dt).name


def test_appended_all_zero_layers_leave_the_bits(ctx):
    shape = (9, 65)
    for L, extra in ((0, 1), (1, 2), (3, 13)):
        for gdt in DT:
            (fr, ly, pl, sg), kw = case(shape, L, np.float32, gdt, "fractional", True, 0)
            a = ctx.temporal_accumulate(fr, ly, pl, sg, **kw)
            zeros = [np.zeros(shape + (4,), gdt) for _ in range(extra)]
            b = ctx.temporal_accumulate(fr, ly + zeros, pl + zeros, sg + [0.5] * extra, **kw)
            assert all(same(x, y) for x, y in zip(a, b)), (L, extra, np.dtype(gdt).name)
