"""CPU: the exact integer answers of np_atrous_exact.py, held against the two float64 checkers and against the conditions that keep
their inputs from becoming trivial.  Every input set of tests/test_gpu_atrous_exact.py passes through here.

    * the integer answer agrees with np_atrous_joint.one_pass / np_atrous_temporal.temporal_pass (float64, real exponentials,
      sigma 0.02) within 1e-6 max(1, |ref|): half an ulp of fp32 at 15 is 4.8e-7;
    * between 30 % and 90 % of the in-image non-centre taps are accepted, at every (layer count, step) in use;
    * dropping any one layer changes the answer somewhere, and so does putting a layer's y or z plane in place of its x plane;
    * numerators stay below 2^24, denominators above 0 (np_atrous_exact.quotient asserts both, and that fp32 holds them);
    * the answer does not depend on the order of the taps or of the frames.

The frames (1, 1) and (5, 7) have no or too few non-centre taps for the second and third condition (at step 8 a 5 x 7 frame has
none); they are held to the first and the fourth, the share and the live slots are asserted from (33, 130) upwards.
"""
import numpy as np
import pytest

import np_atrous_exact as ex
import np_atrous_joint as single
import np_atrous_temporal as temporal

TOL = 1e-6
SIG = ex.SIGMA


def close(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))))


def variants(ly):
    """(name, layers) with one layer dropped, and with one layer's x plane replaced by its y or its z plane."""
    for l in range(len(ly)):
        if len(ly) > 1:
            yield f"without layer {l}", ly[:l] + ly[l + 1:]
        for c in (1, 2):
            # the plane travels as a pattern: plane c's low / high become plane x's own pair
            g = ly[l].copy()
            lo_c, lo_x, hi_x = ly[l][..., c].min(), ly[l][..., 0].min(), ly[l][..., 0].max()
            g[..., 0] = np.where(ly[l][..., c] > lo_c, hi_x, lo_x)
            yield f"layer {l}: x := {'xyz'[c]}", ly[:l] + [g] + ly[l + 1:]


SINGLE_SETS = [(ex.FRAME, L, False, tuple(range(8))) for L in ex.LAYERS] + [(ex.FRAME, L, True, tuple(range(8))) for L in ex.COLOUR_LAYERS] + \
              [(s, L, False, ex.SMALL_PASSES) for s in ex.SMALL for L in ex.LAYERS] + [(ex.WIDE, L, False, ex.WIDE_PASSES) for L in ex.WIDE_LAYERS]


@pytest.mark.parametrize("shape,L,colour,passes", SINGLE_SETS,
                         ids=[f"{s[0]}x{s[1]}-L{L}{'-colour' if c else ''}" for s, L, c, _ in SINGLE_SETS])
def test_single_frame_sets(shape, L, colour, passes):
    fr, ly = ex.single_inputs(shape, L, colour)
    same = ex.single_predicate(shape, L, colour)
    G = [single.widen(l)[..., :3] for l in ly]
    big = shape[0] * shape[1] >= 33 * 130
    for gdt in (np.float16, np.uint8):                      # the other guide dtypes carry the same pattern: one predicate, one answer
        other = ex.equal_on(ex.single_inputs(shape, L, colour, gdt=gdt)[1], fr if colour else None)
        assert np.array_equal(ex.exact_pass(fr, other, 1), ex.single_answer(shape, L, colour, 1))
    assert np.array_equal(ex.single_inputs(shape, L, colour, fdt=np.float16)[0].astype(np.float32), fr)
    changed = [(name, ex.equal_on(v, fr if colour else None)) for name, v in variants(ly)] if big else []
    for i in passes:
        step = 2 ** i
        num, den, acc, off = ex.pass_sums(fr, same, step)
        want = ex.single_answer(shape, L, colour, step)
        assert np.array_equal(want, ex.quotient(num, den))
        ref = single.one_pass(fr.astype(np.float64), G, [SIG] * L, step, SIG * 2.0 ** -i if colour else 0.0)
        assert close(want, ref) <= TOL, (step, close(want, ref))
        assert np.array_equal(want.view(np.uint32), ex.exact_pass(fr, same, step, reverse=True).view(np.uint32))
        if not big:
            continue
        assert 0.30 <= acc / off <= 0.90, (step, acc / off)
        for name, other in changed:
            assert not np.array_equal(ex.exact_pass(fr, other, step), want), (step, name)
        if colour:
            # the colour term is live (without it the answer moves), and alpha is not part of it: another alpha, same accepted taps
            assert not np.array_equal(ex.exact_pass(fr, ex.equal_on(ly), step), want), step
            fr2 = fr.copy()
            fr2[..., 3] = 15 - fr[..., 3]
            n2, d2, _, _ = ex.pass_sums(fr2, ex.equal_on(ly, fr2), step)
            assert np.array_equal(d2, den) and np.array_equal(n2[..., :3], num[..., :3])


@pytest.mark.parametrize("L", ex.LAYERS)
@pytest.mark.parametrize("shape", ex.T_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_temporal_sets(shape, L):
    fr, ly = ex.temporal_inputs(shape, L)
    for k in ex.T_K:
        for t in range(ex.T_FRAMES):
            accepted = ex.equal_across(ly, t)
            num, den, acc, off = ex.temporal_sums(fr, accepted, t, k)
            want = ex.temporal_answer(shape, L, t, k)
            assert np.array_equal(want, ex.quotient(num, den))
            ref = temporal.temporal_pass(fr, ly, [SIG] * L, t, k)
            assert close(want, ref) <= TOL, (k, t, close(want, ref))
            assert np.array_equal(want.view(np.uint32), ex.exact_temporal_pass(fr, accepted, t, k, reverse=True).view(np.uint32))
            assert 0.30 <= acc / off <= 0.90, (k, t, acc / off)
            # the neighbours count: the window's answer is not the lone frame's, and a neighbour's taps are accepted in part
            assert not np.array_equal(want, ex.exact_temporal_pass(fr, accepted, t, 0))
            for f in range(max(0, t - k), min(ex.T_FRAMES - 1, t + k) + 1):
                if f != t:
                    share = np.mean([accepted(f, p, q).mean() for _, _, p, q in ex._taps(shape[0], shape[1], 1, False)])
                    assert 0.05 < share < 0.95, (k, t, f, share)
            if (k, t) != (2, 1):
                continue                                    # the live slots: once per set, on the widest window
            for name, v in variants(ly[0]):
                # the same change in every frame of the sequence
                vs = [dict(variants(ly[f]))[name] for f in range(ex.T_FRAMES)]
                assert not np.array_equal(ex.exact_temporal_pass(fr, ex.equal_across(vs, t), t, k), want), name


def test_the_second_pass_of_the_temporal_case_continues_from_the_exact_level():
    """tests/test_gpu_atrous_exact.py feeds the exact level of pass 0 to pass 1: it is a float32 level like any other, and the
    float64 checker's two-pass result stays within 1e-5 of one_pass on it (the GPU test compares bits with the single-frame
    filter, which the tests above pin at step 2)."""
    shape, L, t, k = ex.T_SHAPES[0], 3, 1, 2
    fr, ly = ex.temporal_inputs(shape, L)
    level = ex.temporal_answer(shape, L, t, k)
    two = temporal.atrous_joint_temporal(fr, ly, [SIG] * L, k, passes=2, first=t, count=1)[0]
    G = [single.widen(l)[..., :3] for l in ly[t]]
    assert close(single.one_pass(level.astype(np.float64), G, [SIG] * L, 2, 0.0), two) <= 1e-5
