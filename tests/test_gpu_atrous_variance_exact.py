"""GPU suite: one variance-guided a-trous pass in every kernel class at every step, bit for bit against exact integer answers
(np_atrous_variance_exact.py; tests/test_atrous_variance_exact_reference.py holds the inputs to their conditions on the CPU).

A grey frame of integers, guides of two values per plane at sigma 0.02, an integer variance plane, sigmaLum = 2^-20 and
epsilon = 2^-10 leave a tap the weight K(o) or 0: the three sums of a pass are integers over 256 or 65536 and colour and variance
are one correctly rounded fp32 quotient each, whichever kernel computes them and in whatever order.  One wrong tap offset, a wrong
address into the variance plane of the comb tile (both chunk sizes: 16 and 8 rows), a w in place of w^2 in the propagation or a
wrong border tap moves bits.  261 rows x 131 columns: a second comb chunk at steps 16 and 32, three tile columns, the last 3 wide;
259 x 258 adds the taps i = +-2 of step 128 inside the image.
"""
import numpy as np
import pytest

import np_atrous_variance_exact as vex

pytestmark = pytest.mark.gpu

GDT = (np.float32, np.float16, np.uint8)
FDT = (np.float32, np.float16)


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def where(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return f"{len(bad)} values differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, exact {want[tuple(bad[0])]!r}"


def run_pass(ctx, shape, L, i, n):
    """Pass i alone on input set (shape, L); n picks the dtypes."""
    fr, v, ly = vex.inputs(shape, L, fdt=FDT[n % 2], gdt=GDT[n % 3])
    return ctx.atrous_variance(fr, v, ly, [vex.SIGMA] * L, passes=1, first_pass=i, sigma_lum=vex.SIGMA_LUM, epsilon=vex.EPSILON,
                               return_variance=True)


@pytest.mark.parametrize("L", vex.LAYERS)
def test_every_step_is_exact(ctx, L):
    for i in range(8):
        gotC, gotV = run_pass(ctx, vex.FRAME, L, i, i + vex.LAYERS.index(L))
        wantC, wantV = vex.answer(vex.FRAME, L, 2 ** i)
        assert same_bits(gotC, wantC), (L, 2 ** i, "colour", where(gotC, wantC))
        assert same_bits(gotV, wantV), (L, 2 ** i, "variance", where(gotV, wantV))


def test_a_wide_frame_is_exact_at_the_largest_steps(ctx):
    for L in vex.WIDE_LAYERS:
        for i in vex.WIDE_PASSES:
            gotC, gotV = run_pass(ctx, vex.WIDE, L, i, i + vex.LAYERS.index(L) + 1)
            wantC, wantV = vex.answer(vex.WIDE, L, 2 ** i)
            assert same_bits(gotC, wantC), (L, 2 ** i, "colour", where(gotC, wantC))
            assert same_bits(gotV, wantV), (L, 2 ** i, "variance", where(gotV, wantV))
