"""GPU suite: one a-trous pass in every kernel class at every step, bit for bit against exact integer answers (np_atrous_exact.py;
tests/test_atrous_exact_reference.py holds the inputs to their conditions on the CPU).

A frame of integers 0 .. 15 and guides of two values per plane at sigma 0.02 leave a tap the weight K(o) or 0, nothing between:
the sums of a pass are integers over 256 and its result is one correctly rounded fp32 quotient, whichever kernel computes it and
in whatever order.  One wrong tap offset, coefficient, layer plane or border tap moves bits.  ctx.atrous_joint(passes=1,
first_pass=i) runs pass i alone on the integer frame, so a pass at step 32 sees the same sharp input as one at step 1.

The frame is 261 rows x 131 columns: the row comb has a second chunk at step 16 (two rows per wave) and at step 32 (one), which
only the residue classes 0 .. 4 of step 32 reach (261 = 8 * 32 + 5); three tile columns, the last 3 wide; the step-32 halo covers a
whole neighbouring tile; steps 64 and 128 still have taps inside the image in both directions.  With 1 .. 5 and 16 layers these are
all rows of the class table of DESIGN 3.10.  Guide and frame dtypes rotate with layer count and step.  A 259 x 258 frame adds what
131 columns cannot hold: the taps i = +-2 of step 128, and with them its corner taps, inside the image.

The exact inputs have no weight strictly between 0 and K(o), so a float64 companion runs the same single passes on HDR noise and
render layers at the suite's sigma sets, within the project's 1e-5 max(1, |ref|).
"""
import numpy as np
import pytest

import guide_format_inputs as gi
import np_atrous_exact as ex
import np_atrous_joint as chk
from conftest import rel_err

pytestmark = pytest.mark.gpu

GDT = (np.float32, np.float16, np.uint8)
FDT = (np.float32, np.float16)
SIGMA_SETS = [(0.5, 0.5, 0.5), (1.0, 2.0, 0.5), (0.25, 0.5, 0.5)]     # test_gpu_atrous_joint.py's
TOL = 1e-5                                             # the project's, for the float64 companion only
WORST = {}


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def where(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return f"{len(bad)} values differ, first at (y, x, c) = {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, exact {want[tuple(bad[0])]!r}"


def run_pass(ctx, shape, L, colour, i, n):
    """Pass i alone on input set (shape, L, colour); n picks the dtypes."""
    fr, ly = ex.single_inputs(shape, L, colour, fdt=FDT[n % 2], gdt=GDT[n % 3])
    return ctx.atrous_joint(fr, ly, [ex.SIGMA] * L, passes=1, first_pass=i, color_sigma=ex.SIGMA if colour else 0.0)


# ---- 1. single frame -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ex.LAYERS)
def test_every_step_is_exact(ctx, L):
    for i in range(8):
        got = run_pass(ctx, ex.FRAME, L, False, i, i + ex.LAYERS.index(L))
        want = ex.single_answer(ex.FRAME, L, False, 2 ** i)
        assert same_bits(got, want), (L, 2 ** i, where(got, want))


@pytest.mark.parametrize("L", ex.COLOUR_LAYERS)
def test_every_step_is_exact_with_the_colour_term(ctx, L):
    """Taps are accepted where labels AND rgb agree (pass i at colorSigma 2^-i: stricter still); the averaged alpha is part of the
    answer, and moves if alpha enters the colour distance or the centre colour comes from another texel."""
    for i in range(8):
        got = run_pass(ctx, ex.FRAME, L, True, i, i + 1 + ex.LAYERS.index(L))
        want = ex.single_answer(ex.FRAME, L, True, 2 ** i)
        assert same_bits(got, want), (L, 2 ** i, where(got, want))


@pytest.mark.parametrize("shape", ex.SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_frames_are_exact(ctx, shape):
    for L in ex.LAYERS:
        for i in ex.SMALL_PASSES:
            got = run_pass(ctx, shape, L, False, i, i + ex.LAYERS.index(L) + 2)
            want = ex.single_answer(shape, L, False, 2 ** i)
            assert same_bits(got, want), (shape, L, 2 ** i, where(got, want))


def test_a_wide_frame_is_exact_at_the_largest_steps(ctx):
    """261 x 131 has no two columns 256 texels apart: the taps i = +-2 of step 128, its corner taps among them, lie inside the
    image only in a frame of more than 256 texels both ways."""
    for L in ex.WIDE_LAYERS:
        for i in ex.WIDE_PASSES:
            got = run_pass(ctx, ex.WIDE, L, False, i, i + ex.LAYERS.index(L) + 1)
            want = ex.single_answer(ex.WIDE, L, False, 2 ** i)
            assert same_bits(got, want), (L, 2 ** i, where(got, want))


def test_float16_output_is_the_packed_exact_answer(ctx):
    shape, L = ex.SMALL[2], 3
    fr, ly = ex.single_inputs(shape, L)
    for i in ex.SMALL_PASSES:
        got = ctx.atrous_joint(fr, ly, [ex.SIGMA] * L, passes=1, first_pass=i, out_dtype=np.float16)
        want = ctx.pack_f16(ex.single_answer(shape, L, False, 2 ** i))
        assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), want.view(np.uint16)), 2 ** i
        assert np.array_equal(want.view(np.uint16), ex.single_answer(shape, L, False, 2 ** i).astype(np.float16).view(np.uint16))


# ---- 2. over neighbouring frames -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", ex.LAYERS)
@pytest.mark.parametrize("shape", ex.T_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_temporal_pass_is_exact(ctx, shape, L):
    for k in ex.T_K:
        n = k + ex.LAYERS.index(L) + ex.T_SHAPES.index(shape)
        fr, ly = ex.temporal_inputs(shape, L, fdt=FDT[n % 2], gdt=GDT[n % 3])
        got = ctx.atrous_joint_temporal(fr, ly, [ex.SIGMA] * L, k=k, passes=1)
        assert len(got) == ex.T_FRAMES
        for t in range(ex.T_FRAMES):
            want = ex.temporal_answer(shape, L, t, k)
            assert same_bits(got[t], want), (shape, L, k, t, where(got[t], want))


@pytest.mark.parametrize("L", [3, 5])
def test_two_temporal_passes_continue_from_the_exact_level(ctx, L):
    shape, k = ex.T_SHAPES[0], 2
    fr, ly = ex.temporal_inputs(shape, L)
    got = ctx.atrous_joint_temporal(fr, ly, [ex.SIGMA] * L, k=k, passes=2)
    for t in range(ex.T_FRAMES):
        want = ctx.atrous_joint(ex.temporal_answer(shape, L, t, k), ly[t], [ex.SIGMA] * L, passes=1, first_pass=1)
        assert same_bits(got[t], want), (L, t, where(got[t], want))


# ---- 3. float64 companion --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 4, 5])
def test_single_passes_against_float64(ctx, L):
    fr = gi.hdr_frames(ex.FRAME, 1, seed=11)[0]
    for i in range(8):
        n = i + L
        sset, cs, gdt = SIGMA_SETS[n % 3], (0.0, 1.0, 4.0)[(n // 3) % 3], (np.float32, np.float16)[n % 2]
        sets = [gi.render_layers(ex.FRAME, 1, gdt, seed=12 + s)[0] for s in range((L + 2) // 3)]
        ly, sg = [sets[l // 3][l % 3] for l in range(L)], [sset[l % 3] for l in range(L)]
        got = ctx.atrous_joint(fr, ly, sg, passes=1, first_pass=i, color_sigma=cs)
        ref = chk.atrous_joint(fr, ly, sg, passes=1, first_pass=i, color_sigma=cs)
        err = rel_err(got, ref)
        key = f"L={L}, step {2 ** i}"
        WORST[key] = err
        print(f"one pass at step {2 ** i}, L={L}, sigmas={sset}, colour={cs}, guides={np.dtype(gdt).name}: {err:.3e}")
        assert np.isfinite(got).all()
        assert err <= TOL, (L, 2 ** i, sset, cs, err)


def test_report_worst_errors():
    for L in (1, 4, 5):
        print(f"worst error of one pass against float64, L={L}: " + ", ".join(f"step {2 ** i}: {WORST.get(f'L={L}, step {2 ** i}', float('nan')):.2e}" for i in range(8)))
