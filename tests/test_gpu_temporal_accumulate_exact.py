"""GPU suite: the recursive temporal accumulation (include/mi_denoise.h, section a4j) against exact answers
(tests/np_temporal_accumulate_exact.py): grey integer frames and histories, label layers that weigh 1 or 0, motion in integers
and halves, history lengths 1, 3 and 7 with alpha below 1/8.  Colour, moments, N' and Vt must come out BIT FOR BIT -- which pins
the tap offsets, their order, which texel each weight meets, the skipped taps and the unnormalised N'."""
import numpy as np
import pytest

import np_temporal_accumulate_exact as ex
from test_gpu_atrous_bounds import same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L", [1, 5, 16])
@pytest.mark.parametrize("shape", [(130, 35), (131, 261)], ids=lambda s: f"{s[1]}x{s[0]}")
def test_bit_for_bit(ctx, shape, L):
    for seed, (alpha, alpha_m, hmax) in enumerate(((0.0625, 0.1, 32), (0.1, 0.0625, 4))):
        fr, hist, mv = ex.grey_frame(shape, seed), ex.history(shape, seed), ex.motion(shape, seed)
        ly, pl = ex.label_layers(shape, L, 1), ex.label_layers(shape, L, 0)
        col, st, vt, rejected = ex.temporal_accumulate_exact(fr, ly, pl, hist, mv, alpha, alpha_m, hmax)
        assert 0.05 < rejected < 0.95, rejected
        for gdt in (np.uint8, np.float32):
            lyd, pld = ([g if gdt == np.uint8 else (g / np.float32(255)).astype(np.float32) for g in gs] for gs in (ly, pl))
            got = ctx.temporal_accumulate(fr, lyd, pld, [ex.SIGMA] * L, hist=hist, motion=mv, alpha=alpha, alpha_moments=alpha_m,
                                          history_max=hmax)
            for g, want, what in zip(got, (col, st, vt), ("colour", "state", "Vt")):
                assert same(g, want), (shape, L, seed, np.dtype(gdt).name, what, int((g != want).sum()))
