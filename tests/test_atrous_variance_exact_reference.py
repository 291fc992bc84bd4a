"""CPU: the exact integer answers of np_atrous_variance_exact.py, held to the conditions that keep the inputs of
tests/test_gpu_atrous_variance_exact.py from becoming trivial:

    * the integer answer agrees with the float64 checker (np_atrous_variance.one_pass: real exponentials, sigma 0.02,
      sigmaLum 2^-20, epsilon 2^-10) within 1e-6 max(1, |ref|), colour and variance;
    * between 30 % and 90 % of the in-image non-centre taps are accepted at every (layer count, step) in use;
    * every layer slot and plane is live, and so is the grey: dropping a layer, moving a layer's y or z plane into its x plane, or
      taking the luminance term away changes the answer;
    * V_out differs from V_in on most pixels -- at step 128 on the 261 x 131 frame a pixel has ONE in-image non-centre tap (131
      columns hold no two texels 128 apart but for six columns, 261 rows one row 128 away), so the share of changed pixels cannot
      exceed the share of accepted taps, which may be as low as 30 %: there, and wherever a pixel has fewer than two such taps
      on average, the condition is held on the pixels that have an accepted tap at all (more than 90 % of them change);
    * the answer does not depend on the order of the taps.
"""
import numpy as np
import pytest

import np_atrous_exact as ex
import np_atrous_variance as chk
import np_atrous_variance_exact as vex
from test_atrous_exact_reference import variants

TOL = 1e-6

SETS = [(vex.FRAME, L, tuple(range(8))) for L in vex.LAYERS] + [(vex.WIDE, L, vex.WIDE_PASSES) for L in vex.WIDE_LAYERS]


def close(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))))


@pytest.mark.parametrize("shape,L,passes", SETS, ids=[f"{s[0]}x{s[1]}-L{L}" for s, L, _ in SETS])
def test_exact_sets(shape, L, passes):
    fr, v, ly = vex.inputs(shape, L)
    same = vex.predicate(shape, L)
    assert np.array_equal(fr[..., 0], fr[..., 1]) and np.array_equal(fr[..., 0], fr[..., 2]) and len(np.unique(fr[..., 0])) >= 4
    assert np.array_equal(vex.inputs(shape, L, fdt=np.float16)[0].astype(np.float32), fr)
    for gdt in (np.float16, np.uint8):                      # the other guide dtypes carry the same pattern: one predicate, one answer
        other = ex.equal_on(vex.inputs(shape, L, gdt=gdt)[2], fr)
        got = vex.exact_pass(fr, v, other, 1)
        assert np.array_equal(got[0], vex.answer(shape, L, 1)[0]) and np.array_equal(got[1], vex.answer(shape, L, 1)[1])
    changed = [(name, ex.equal_on(x, fr)) for name, x in variants(ly)] + [("no luminance term", ex.equal_on(ly))]
    Gs = chk._scaled(ly, [vex.SIGMA] * L)
    for i in passes:
        step = 2 ** i
        wantC, wantV = vex.answer(shape, L, step)
        refC, refV = chk.one_pass(fr.astype(np.float64), v.astype(np.float64), Gs, step, vex.SIGMA_LUM, vex.EPSILON)
        assert close(wantC, refC) <= TOL and close(wantV, refV) <= TOL, (step, close(wantC, refC), close(wantV, refV))
        _, den, _, acc, off = vex.sums(fr, v, same, step)
        assert 0.30 <= acc / off <= 0.90, (step, acc / off)
        revC, revV = vex.exact_pass(fr, v, same, step, reverse=True)
        assert np.array_equal(revC.view(np.uint32), wantC.view(np.uint32)) and np.array_equal(revV.view(np.uint32), wantV.view(np.uint32))
        for name, other in changed:
            gotC, gotV = vex.exact_pass(fr, v, other, step)
            assert not np.array_equal(gotC, wantC) and not np.array_equal(gotV, wantV), (step, name)
        if off / v.size >= 2:
            assert (wantV != v).mean() > 0.5, step
        else:
            has = den > 36                                  # more than the centre tap's 6 * 6
            assert has.mean() >= 0.30 and (wantV != v)[has].mean() > 0.9, (step, has.mean())
