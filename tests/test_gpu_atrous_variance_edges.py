"""GPU suite: the variance-guided a-trous filter (include/mi_denoise.h, section a4i) where test_gpu_atrous_variance.py does not
look, every result against the float64 checker (np_atrous_variance.py), which test_atrous_variance_checker_edges.py holds to
per-pixel loops on exactly such frames.  The inputs are atrous_variance_edge_inputs.py's; test_atrous_variance_edge_inputs.py holds
every finite case to the 2e-6 well-posedness bound on the CPU.  Tolerances are the header's: colour 1e-5 max(1, |ref|), variance
1e-5 max(1, max V_ref), moments 1e-5 max(1, M2_ref).

    1. tiny and seam frames: narrower than a wave, shorter than the step (whole residue classes of the comb leave at once),
       shorter than a chunk of 8 or 16 comb rows, 1 x 1, steps wider than the frame; 1 .. 16 layers, every frame and guide format.
    2. every chunk count: heights 1 .. 40 at width 67 and tall narrow frames, one pass a call through the raw C call into NaN-filled
       outputs between guard bands: no NaN left, the bands intact, the result that of float64.
    3. value range: radiance 1/64, 16 and 1024 times the usual; the dim frame against itself times 2^10 bit for bit; a converged frame.
    4. non-finite texels: the non-finite pixels are those of IEEE arithmetic on the header's formula, the others are right.
    5. the moments at every tile-row count, as 2.
"""
import ctypes

import numpy as np
import pytest

import atrous_variance_edge_inputs as evi
import atrous_variance_inputs as avi
import image_denoising_filter_amd as mid
import np_atrous_variance as chk
from conftest import rel_err
from test_gpu_atrous_bounds import FMT, Banded, same

pytestmark = pytest.mark.gpu

TOL = 1e-5
WORST = {}


def var_err(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref)) / max(1.0, ref.max()))


def klass(L, first, n):
    """The kernel classes of passes first .. first + n - 1 with L layers."""
    comb, glob = L <= 4 and first <= 5, L > 4 or first + n > 6
    return "comb" if not glob else "global" if not comb else "comb, then global"


def note(section, L, first, n, ec, ev):
    key = f"{section}, {klass(L, first, n)}"
    wc, wv = WORST.get(key, (0.0, 0.0))
    WORST[key] = (max(wc, ec), max(wv, ev))


def nan_plane(shape):
    return np.full(shape, np.nan, np.float32)


def raw_pass(ctx, fr, v0, ly, sg, first, sl, eps):
    """One pass through the C call: `out` and var_out hold NaN before it and lie between guard bands of sentinel bytes."""
    h, w = fr.shape[:2]
    d_in, d_vin, d_l = ctx.upload(fr), ctx.upload(v0), [ctx.upload(l) for l in ly]
    d_out = Banded(ctx, h * w * 16, nan_plane((h, w, 4)), None, seed=40)
    d_vout = Banded(ctx, h * w * 4, nan_plane((h, w)), None, seed=42)
    p = mid.AtrousVarianceParams(w, h, first, 1, sl, eps, mid.api.fmt_with_guide(FMT[fr.dtype], FMT[ly[0].dtype]))
    rc = mid.lib.mid_atrous_variance(ctx.handle, ctypes.byref(p), (ctypes.c_float * 16)(*sg), d_in.ptr, d_vin.ptr,
                                     (ctypes.c_void_p * 17)(*[d.ptr for d in d_l]), len(ly), d_out.ptr, mid.FMT_RGBA32F, d_vout.ptr, None, None)
    assert rc == 0, mid.lib.mid_last_error()
    ctx.sync()
    assert d_out.bands_intact(), "a store beside out"
    assert d_vout.bands_intact(), "a store beside var_out"
    return d_out.middle((h, w, 4), np.float32), d_vout.middle((h, w), np.float32)


def raw_moments(ctx, frames, layers, sg, k, t):
    """The moments through the C call into a NaN-filled var_out between guard bands."""
    h, w = frames[0].shape[:2]
    n, L = len(frames), len(layers[0])
    d_fr = [ctx.upload(f) for f in frames]
    d_l = [ctx.upload(l) for ls in layers for l in ls]
    d_var = Banded(ctx, h * w * 4, nan_plane((h, w)), None, seed=50)
    p = mid.AtrousMomentsParams(w, h, mid.api.fmt_with_guide(FMT[frames[0].dtype], FMT[layers[0][0].dtype]))
    rc = mid.lib.mid_atrous_moments(ctx.handle, ctypes.byref(p), (ctypes.c_float * 16)(*sg), (ctypes.c_void_p * n)(*[d.ptr for d in d_fr]),
                                    (ctypes.c_void_p * len(d_l))(*[d.ptr for d in d_l]), L, n, k, t, d_var.ptr, None)
    assert rc == 0, mid.lib.mid_last_error()
    ctx.sync()
    assert d_var.bands_intact(), "a store beside the moments' plane"
    return d_var.middle((h, w), np.float32)


# ---- 1. tiny and seam frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", evi.TINY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiny_and_seam_frames_against_float64(ctx, shape):
    for c in evi.tiny_cases(shape):
        _, L, fdt, gdt, first, n, sl, eps = c
        fr, v0, ly, sg = evi.case_inputs(c)
        refC, refV = evi.case_reference(c)
        gotC, gotV = ctx.atrous_variance(fr, v0, ly, sg, passes=n, first_pass=first, sigma_lum=sl, epsilon=eps, return_variance=True)
        ec, ev = rel_err(gotC, refC), var_err(gotV, refV)
        note("tiny and seam frames", L, first, n, ec, ev)
        print(f"{evi.case_id(c)}: colour {ec:.3e}, variance {ev:.3e}")
        assert gotC.shape == shape + (4,) and gotV.shape == shape and np.isfinite(gotC).all() and np.isfinite(gotV).all(), evi.case_id(c)
        assert ec <= TOL and ev <= TOL, (evi.case_id(c), ec, ev)


# ---- 2. every chunk count, every pixel written ---------------------------------------------------------------------------------------
def check_raw(ctx, c, section):
    _, L, _, _, first, n, sl, eps = c
    fr, v0, ly, sg = evi.case_inputs(c)
    refC, refV = evi.case_reference(c)
    gotC, gotV = raw_pass(ctx, fr, v0, ly, sg, first, sl, eps)
    assert not np.isnan(gotC).any() and not np.isnan(gotV).any(), (evi.case_id(c), "a pixel was not written",
                                                                   np.argwhere(np.isnan(gotC).any(-1) | np.isnan(gotV))[:4].tolist())
    ec, ev = rel_err(gotC, refC), var_err(gotV, refV)
    note(section, L, first, n, ec, ev)
    assert ec <= TOL and ev <= TOL, (evi.case_id(c), ec, ev)
    return ec, ev


@pytest.mark.parametrize("first", evi.SWEEP_FIRST)
@pytest.mark.parametrize("L", evi.SWEEP_LAYERS)
def test_every_height_up_to_40_is_written_whole(ctx, L, first):
    worst = (0.0, 0.0)
    for h in evi.SWEEP_HEIGHTS:
        worst = tuple(map(max, worst, check_raw(ctx, evi.one_pass_case((h, evi.SWEEP_WIDTH), L, first), "heights 1..40 x 67")))
    print(f"L={L} step {2 ** first}: 40 heights, worst colour {worst[0]:.3e}, variance {worst[1]:.3e}")


@pytest.mark.parametrize("shape", evi.TALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tall_narrow_frames_are_written_whole(ctx, shape):
    worst = (0.0, 0.0)
    for L in evi.TALL_LAYERS:
        for first in evi.TALL_FIRST:
            worst = tuple(map(max, worst, check_raw(ctx, evi.one_pass_case(shape, L, first), "tall narrow frames")))
    print(f"{shape}: 20 calls, worst colour {worst[0]:.3e}, variance {worst[1]:.3e}")


# ---- 3. value range --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", evi.SCALES, ids=lambda s: f"x{s:g}")
def test_scaled_radiance_against_float64(ctx, scale):
    for c in (c for c in evi.SCALED if c[0] == scale):
        _, L, sl, first, n = c
        fr, v0, ly, sg, eps = evi.scaled_inputs(c)
        refC, refV = evi.scaled_reference(c)
        gotC, gotV = ctx.atrous_variance(fr, v0, ly, sg, passes=n, first_pass=first, sigma_lum=sl, epsilon=eps, return_variance=True)
        ec, ev = rel_err(gotC, refC), var_err(gotV, refV)
        note(f"radiance x {scale:g}", L, first, n, ec, ev)
        print(f"{evi.scaled_id(c)}: colour {ec:.3e}, variance {ev:.3e} (max |C_ref| {np.abs(refC).max():.4g}, max V_ref {refV.max():.4g})")
        assert np.isfinite(gotC).all() and np.isfinite(gotV).all(), evi.scaled_id(c)
        assert ec <= TOL and ev <= TOL, (evi.scaled_id(c), ec, ev)


def where(got, want):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    return f"{len(bad)} values differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r}, scaled {want[tuple(bad[0])]!r}" if len(bad) else ""


@pytest.mark.parametrize("fdt", [np.float32, np.float16], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("L", evi.SCALED_LAYERS)
def test_a_dim_frame_times_a_power_of_two_scales_every_bit(ctx, L, fdt):
    """max(1, |ref|) makes the header's bound loose for a dim frame; this is tight.  Frame (rgb and alpha) times 2^10, var_in times
    2^20, epsilon times 2^10: every intermediate of the header's formula is multiplied by an exact power of two and the weights
    keep their bits, so colour is ldexp(colour, 10) and V is ldexp(V, 20) of the unscaled call, in the comb and the global class."""
    dim = evi.scaled_frames(1.0 / 64.0, fdt)[1]
    big = dim * fdt(1024)
    v = evi.scaled_v0(1.0 / 64.0, L)
    vb = v * np.float32(2.0 ** 20)
    eps = np.float32(1e-3 / 64.0)
    ly, sg = avi.layers_of(evi.RANGE_SHAPE, L, np.float32, 1), avi.sigmas_of(L)
    for first, n in evi.SCALED_RANGES:
        for sl in (4.0, 0.25):
            kw = dict(passes=n, first_pass=first, sigma_lum=sl, return_variance=True)
            aC, aV = ctx.atrous_variance(dim, v, ly, sg, epsilon=float(eps), **kw)
            bC, bV = ctx.atrous_variance(big, vb, ly, sg, epsilon=float(eps * np.float32(1024)), **kw)
            assert np.isfinite(aC).all() and np.isfinite(aV).all() and aV.min() >= 0 and aV.max() > 0
            assert same(np.ldexp(aC, 10), bC), (L, first, n, sl, "colour", where(bC, np.ldexp(aC, 10)))
            assert same(np.ldexp(aV, 20), bV), (L, first, n, sl, "variance", where(bV, np.ldexp(aV, 20)))


@pytest.mark.parametrize("L", [2, 4, 5])
def test_the_moments_of_a_dim_frame_scale_every_bit(ctx, L):
    sg = avi.sigmas_of(L)
    ly = [avi.layers_of(evi.RANGE_SHAPE, L, np.float32, f) for f in range(avi.N_FRAMES)]
    for fdt in (np.float32, np.float16):
        dim = evi.scaled_frames(1.0 / 64.0, fdt)
        big = [f * fdt(1024) for f in dim]
        for k in (0, 1):
            a, b = ctx.atrous_moments(dim, ly, sg, k=k, t=1), ctx.atrous_moments(big, ly, sg, k=k, t=1)
            assert np.isfinite(a).all() and a.max() > 0
            assert same(np.ldexp(a, 20), b), (L, np.dtype(fdt).name, k, where(b, np.ldexp(a, 20)))


@pytest.mark.parametrize("L", [1, 5])
def test_a_converged_frame_stays_constant_with_zero_variance(ctx, L):
    """V = 0 everywhere: the luminance scale is log2(e) / epsilon = 1.4e6, and every luminance difference it meets is exactly 0."""
    shape = evi.RANGE_SHAPE
    const = np.array([0.3, 2.5, 0.01, 0.7], np.float32)
    fr = np.broadcast_to(const, shape + (4,)).copy()
    gotC, gotV = ctx.atrous_variance(fr, np.zeros(shape, np.float32), avi.layers_of(shape, L, np.float32, 1), avi.sigmas_of(L), passes=5,
                                     sigma_lum=4.0, epsilon=1e-6, return_variance=True)
    assert np.isfinite(gotC).all() and np.isfinite(gotV).all()
    ec = rel_err(gotC, np.broadcast_to(const.astype(np.float64), shape + (4,)))
    print(f"L={L}: a constant frame after five passes is off by {ec:.3e}")
    assert ec <= TOL
    assert np.array_equal(gotV, np.zeros(shape, np.float32)), np.abs(gotV).max()


# ---- 4. non-finite texels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", evi.NONFINITE, ids=evi.nonfinite_id)
def test_non_finite_texels_reach_the_pixels_ieee_arithmetic_says(ctx, case):
    L, first, n = case
    fr, v0, ly, sg = evi.nonfinite_inputs(case)
    refC, refV = evi.nonfinite_reference(case)
    gotC, gotV = ctx.atrous_variance(fr, v0, ly, sg, passes=n, first_pass=first, sigma_lum=4.0, epsilon=1e-3, return_variance=True)
    badC, badV = ~np.isfinite(refC), ~np.isfinite(refV)
    for ch in range(4):
        diff = np.argwhere(~np.isfinite(gotC[..., ch]) != badC[..., ch])
        assert len(diff) == 0, (evi.nonfinite_id(case), f"channel {ch}", len(diff), diff[:4].tolist())
    diff = np.argwhere(~np.isfinite(gotV) != badV)
    assert len(diff) == 0, (evi.nonfinite_id(case), "variance", len(diff), diff[:4].tolist())
    ec = rel_err(gotC[~badC], refC[~badC])
    ev = float(np.max(np.abs(gotV[~badV].astype(np.float64) - refV[~badV])) / max(1.0, refV[~badV].max()))
    note("non-finite texels, the finite pixels", L, first, n, ec, ev)
    print(f"{evi.nonfinite_id(case)}: {badC.any(-1).sum()} pixels with a non-finite channel, {badV.sum()} non-finite variances; "
          f"the others: colour {ec:.3e}, variance {ev:.3e}")
    assert ec <= TOL and ev <= TOL, (evi.nonfinite_id(case), ec, ev)


# ---- 5. the moments at every tile-row count ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", evi.SWEEP_LAYERS)
def test_the_moments_are_written_whole_at_every_height_up_to_35(ctx, L):
    sg = avi.sigmas_of(L)
    worst = 0.0
    for h in range(1, 36):
        shape = (h, evi.SWEEP_WIDTH)
        fr = [avi.frame_of(shape, f) for f in range(avi.N_FRAMES)]
        ly = [avi.layers_of(shape, L, np.float32, f) for f in range(avi.N_FRAMES)]
        got = raw_moments(ctx, fr, ly, sg, 1, 1)
        ref, m2 = chk.moments(fr, ly, sg, k=1, t=1)
        assert not np.isnan(got).any(), (L, h, "a pixel was not written", np.argwhere(np.isnan(got))[:4].tolist())
        err = float(np.max(np.abs(got.astype(np.float64) - ref) / np.maximum(1.0, m2)))
        worst = max(worst, err)
        assert got.min() >= 0 and err <= TOL, (L, h, err)
    key = f"moments at heights 1..35 x 67, {'LDS tiles' if L <= 4 else 'global taps'}"
    WORST[key] = max(WORST.get(key, (0.0,)), (worst,))
    print(f"L={L}: 35 heights, worst {worst:.3e}")


def test_report_worst_errors():
    for k in sorted(WORST):
        print(f"worst error against float64, {k}: " + ", ".join(f"{e:.3e}" for e in WORST[k]) + (" (colour, variance)" if len(WORST[k]) == 2 else ""))
