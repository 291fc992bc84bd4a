"""CPU: the inputs that tests/test_gpu_atrous_variance_edges.py asserts on (atrous_variance_edge_inputs.py) meet their conditions,
by the float64 checker alone.

Every finite case is well-posed by the measure of test_the_inputs_of_the_gpu_test_are_well_posed: the float64 formula moves by no
more than 2e-6 max(1, |ref|) when every level and variance plane is rounded to fp32 after each pass, so that the 1e-5 the GPU test
asserts is the filter's arithmetic and not the conditioning of the input.  The bound is a condition on the inputs; nothing here
knows what a kernel returns.  The non-finite cases spread far enough to be a test and not so far that nothing finite is left.
"""
import numpy as np
import pytest

import atrous_variance_edge_inputs as evi
import atrous_variance_inputs as avi
import np_atrous_variance as chk

BOUND = 2e-6


def _hold(cases, reference, name):
    worst = (0.0, 0.0)
    for c in cases:
        ref, ref32 = reference(c), reference(c, True)
        assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and ref[1].min() >= 0, c
        e = evi.posedness(ref, ref32)
        worst = max(worst, e)
        assert e[0] <= BOUND and e[1] <= BOUND, (c, e)
    print(f"{name}: {len(cases)} cases, rounding the levels moves the formula by at most {worst[0]:.2e} (colour, variance {worst[1]:.2e})")


def test_the_tables_are_what_the_gpu_tests_expect():
    assert len(evi.TINY) == 300 and len(set(evi.TINY)) == 300
    for s in evi.TINY_SHAPES:
        cs = evi.tiny_cases(s)
        assert {(c[2], c[3]) for c in cs} == {(a, b) for a in evi.DT for b in evi.DT}        # every pair of dtypes on every shape
        assert {(c[6], c[7]) for c in cs} == set(evi.LUM)
    assert {(c[2], c[6]) for c in evi.TINY} == {(a, sl) for a in evi.DT for sl, _ in evi.LUM}
    assert len(evi.SWEEP) == 480 and len(evi.TALL) == 60 and len(evi.SCALED) == 81 and len(evi.NONFINITE) == 8
    # steps wider than the frame, shorter than the step, shorter than one chunk of 8 comb rows
    assert any(2 ** (c[4] + c[5] - 1) > max(c[0]) for c in evi.TINY) and any(c[0][0] < 2 ** c[4] for c in evi.TINY + evi.TALL)
    assert any(-(-c[0][0] // 2 ** c[4]) < 8 for c in evi.TALL) and any(-(-c[0][0] // 2 ** c[4]) > 16 for c in evi.TALL)


@pytest.mark.parametrize("shape", evi.TINY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny_and_seam_frames_are_well_posed(shape):
    _hold(evi.tiny_cases(shape), evi.case_reference, f"{shape}")


def test_the_height_sweep_is_well_posed():
    _hold(evi.SWEEP, evi.case_reference, "heights 1..40 x 67")


def test_tall_narrow_frames_are_well_posed():
    _hold(evi.TALL, evi.case_reference, "tall frames")


@pytest.mark.parametrize("scale", evi.SCALES, ids=lambda s: f"x{s:g}")
def test_scaled_frames_are_well_posed(scale):
    _hold([c for c in evi.SCALED if c[0] == scale], evi.scaled_reference, f"scale {scale:g}")
    fr = evi.scaled_frames(scale)[1]
    assert np.array_equal(fr[..., :3].astype(np.float64), avi.frame_of(evi.RANGE_SHAPE, 1)[..., :3].astype(np.float64) * scale)   # exact
    assert np.array_equal(fr[..., 3], avi.frame_of(evi.RANGE_SHAPE, 1)[..., 3])
    v = [evi.scaled_v0(scale, L).max() for L in evi.SCALED_LAYERS]
    print(f"scale {scale:g}: radiance up to {fr[..., :3].max():.4g}, V_0 up to {max(v):.4g}")
    if scale == 1024.0:
        assert fr[..., :3].max() > 2000 and max(v) > 1e4


def test_the_power_of_two_frames_scale_exactly():
    for dt in (np.float32, np.float16):
        dim = evi.scaled_frames(1.0 / 64.0, dt)[1]
        big = dim * dt(1024)
        assert big.dtype == dt and np.isfinite(big).all()
        assert np.array_equal(big.astype(np.float64), dim.astype(np.float64) * 1024.0)
        assert dim[..., :3].max() < 0.25
    for L in evi.SCALED_LAYERS:
        v = evi.scaled_v0(1.0 / 64.0, L)
        vb = v * np.float32(2.0 ** 20)
        assert np.array_equal(vb.astype(np.float64), v.astype(np.float64) * 2.0 ** 20) and np.isfinite(vb).all()
        assert v[v > 0].min() > 1e-30                          # no subnormal variance: nothing the scaling could round
    assert np.float32(np.float32(1e-3 / 64.0) * np.float32(1024)) == np.float32(1e-3 / 64.0) * 1024.0


@pytest.mark.parametrize("case", evi.NONFINITE, ids=evi.nonfinite_id)
def test_non_finite_cases_spread_but_leave_half_the_frame(case):
    fr, v0, ly, sg = evi.nonfinite_inputs(case)
    assert (~np.isfinite(fr)).sum() == 6 and (~np.isfinite(v0)).sum() == 4 and (v0 == -1).sum() == 2
    for kinds in ([fr[y, x, c] for y, x, c, _ in evi.NF_COLOUR], [v0[y, x] for y, x, _ in evi.NF_VARIANCE]):
        for half in (kinds[:3], kinds[3:]):                     # one of each kind on the seam, one at a corner
            assert sorted(map(repr, map(float, half))) == sorted(map(repr, map(float, kinds[:3])))
    assert all(x == 64 for _, x, _, _ in evi.NF_COLOUR[:3]) and all(x == 64 for _, x, _ in evi.NF_VARIANCE[:3])
    corners = {(0, 0), (0, 128), (39, 0), (39, 128)}
    assert all((y, x) in corners for y, x, _, _ in evi.NF_COLOUR[3:]) and all((y, x) in corners for y, x, _ in evi.NF_VARIANCE[3:])
    C, V = evi.nonfinite_reference(case)
    bad = ~np.isfinite(C).all(-1) | ~np.isfinite(V)
    print(f"{evi.nonfinite_id(case)}: {bad.sum()} of {bad.size} pixels are non-finite")
    assert bad.sum() >= 20 and 2 * bad.sum() <= bad.size
    # Where a negative variance enters vt, vt is away from 0 by a margin, in every pass: sqrtf(vt) is a NaN or not in fp32 as in
    # float64, whatever the rounding of the nine-term sum.  And the -1 texels do make their own vt negative.
    levels = []
    chk.atrous_variance(fr, v0, ly, sg, passes=case[2], first_pass=case[1], sigma_lum=4.0, epsilon=1e-3, levels=levels)
    with np.errstate(all="ignore"):
        for Vi in [v0.astype(np.float64)] + [lv[1] for lv in levels[:-1]]:
            vt, va = chk.smooth_variance(Vi), chk.smooth_variance(np.abs(Vi))
            mixed = np.isfinite(vt) & (vt != va)
            assert np.all(np.abs(vt[mixed]) >= 1e-4 * va[mixed]), np.abs(vt[mixed] / va[mixed]).min()
    vt = chk.smooth_variance(v0.astype(np.float64))
    assert all(vt[y, x] < -1e-2 for y, x, val in evi.NF_VARIANCE if val == -1.0)
