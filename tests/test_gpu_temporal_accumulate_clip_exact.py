"""GPU suite: mid_temporal_accumulate_clip (section a4m) against answers that are exact, bit for bit.

The construction is tests/np_temporal_accumulate_exact.py's, imported -- grey integer frames and histories, label layers, motion in
integers and halves, so the sums are exact in fp32 in any order -- with integer clip planes; the clip and what follows it are a chain
of single fp32 operations that tests/np_temporal_accumulate_clip_exact.py evaluates bit-true (and that
tests/test_temporal_accumulate_clip_checker.py holds to the imported module wherever nothing is clipped).  Colour, moments and N' must
have the evaluation's bits.
"""
import numpy as np
import pytest

import np_temporal_accumulate_exact as ex
from np_temporal_accumulate_clip_exact import clip_planes, temporal_accumulate_clip_exact
from test_gpu_atrous_bounds import same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(130, 35), (131, 261)], ids=lambda s: f"{s[1]}x{s[0]}")       # 35 x 130 and 261 x 131
def test_colour_moments_and_length_bit_for_bit(ctx, shape):
    for seed, L, (alpha, alpha_m, hmax) in ((1, 0, (0.1, 0.05, 8)), (2, 2, (0.1, 0.05, 8)), (3, 4, (0.0625, 0.25, 4)), (4, 3, (0.2, 0.2, 32))):
        fr, hist, mv = ex.grey_frame(shape, seed), ex.history(shape, seed), ex.motion(shape, seed)
        ly, pl = ex.label_layers(shape, L, 1), ex.label_layers(shape, L, 0)
        lo, hi = clip_planes(shape, seed)
        colour, state, Vt, share = temporal_accumulate_clip_exact(fr, ly, pl, hist, mv, alpha, alpha_m, hmax, lo, hi)
        assert 0.2 < share < 0.98, share
        got = ctx.temporal_accumulate(fr, ly, pl, [ex.SIGMA] * L, hist=hist, motion=mv, alpha=alpha, alpha_moments=alpha_m, history_max=hmax, clip_lo=lo, clip_hi=hi)
        assert same(got[0], colour), (seed, "colour")
        assert same(got[1], state), (seed, "moments and N'")
        assert same(got[2], Vt), (seed, "the temporal variance")
        plain = ctx.temporal_accumulate(fr, ly, pl, [ex.SIGMA] * L, hist=hist, motion=mv, alpha=alpha, alpha_moments=alpha_m, history_max=hmax)
        assert not same(plain[0], got[0]) and same(plain[1][..., 2], got[1][..., 2]), "the clip moves the colour and leaves N'"
