"""CPU suite: the inputs of the GPU tests of the recursive temporal accumulation (tests/temporal_accumulate_inputs.py) must not let
those tests pass vacuously.  On the 261 x 131 moving-label input the float64 checker must see a history that is believed
(S > 0.5) on at least a fifth of the pixels, rejected outright (S == 0) on at least a twentieth, and half believed (0 < S < 0.5)
on at least a tenth -- with every motion field and every layer count from three up.  An input that misses one of these is changed;
the bounds stay."""
import numpy as np
import pytest

import temporal_accumulate_inputs as tai
from np_temporal_accumulate import tap_geometry, temporal_accumulate

SHAPE = (131, 261)


@pytest.mark.parametrize("L", [3, 5, 16])
@pytest.mark.parametrize("motion", tai.MOTIONS)
def test_the_history_is_believed_rejected_and_half_believed(motion, L):
    r = temporal_accumulate(tai.frame_of(SHAPE, 1), tai.layers_of(SHAPE, L, np.uint8, 1), tai.layers_of(SHAPE, L, np.uint8, 0), tai.sigmas_of(L),
                            hist=tai.history_of(SHAPE), motion=tai.motion_of(SHAPE, motion))
    S = r["S"]
    full, none, half = (S > 0.5).mean(), (S == 0).mean(), ((S > 0) & (S < 0.5)).mean()
    print(f"{motion} L={L}: S > 0.5 on {full:.3f}, S == 0 on {none:.3f}, 0 < S < 0.5 on {half:.3f} of the pixels")
    assert full >= 1 / 5 and none >= 1 / 20 and half >= 1 / 10, (full, none, half)
    assert S.max() <= 1.0 + 1e-12


def test_the_label_layer_alone_weighs_one_or_nothing():
    r = temporal_accumulate(tai.frame_of(SHAPE, 1), tai.layers_of(SHAPE, 1, np.float32, 1), tai.layers_of(SHAPE, 1, np.float32, 0), tai.sigmas_of(1),
                            hist=tai.history_of(SHAPE))
    assert set(np.unique(r["S"])) == {0.0, 1.0}


def test_the_motion_fields_take_every_kind_of_tap():
    h, w = SHAPE
    for kind, fractional in (("integer", False), ("fractional", True), ("smooth", True)):
        m = tai.motion_of(SHAPE, kind)
        ok, x0, y0, fx, fy = tap_geometry(h, w, m)
        assert np.abs(m).max() <= 6 and bool(fx.any() or fy.any()) == fractional
        assert (~ok).any() or ((x0 + 1)[ok] >= w).any() or (y0[ok] < 0).any(), kind      # some taps lie beyond the frame
    # the smooth field points off the frame on all four sides: the skip rule is exercised at every edge
    ok, x0, y0, fx, fy = tap_geometry(h, w, tai.motion_of(SHAPE, "smooth"))
    assert (x0[ok] < 0).any() and (x0[ok] + 1 >= w).any() and (y0[ok] < 0).any() and (y0[ok] + 1 >= h).any()
