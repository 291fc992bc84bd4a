"""GPU suite: frames past 262 144 rows -- a second grid dimension of 65 538 workgroups, above the 65 536 the device reports as
hipDeviceAttributeMaxGridDimY -- in the kernels that launch dim3(cdiv(w, 64), cdiv(h, 4)) and dim3(cdiv(w, 16), cdiv(h, 16)).

The recipe is tests/tall_inputs.py's (held to its conditions by tests/test_tall_inputs_args.py): every plane repeats a pattern of 37
rows, tiled on the device, so EVERY row of the tall output is compared -- with the output of a small frame of the same pattern, indexed
by row_map on the device.  A block index that wrapped at 65 536 would store another phase of the pattern over the first rows.

    * Four rows per workgroup, h = 262 149, widths 3 and 65: mid_temporal_accumulate with and without the clip box (label layers,
      history planes, motion of up to 3 rows in integers and halves); one pass of mid_atrous_joint, of mid_atrous_variance and of
      mid_atrous_joint_temporal with five layers (their global classes); mid_median_filter with five layers (its global class: the
      guide and four all-zero layers).  Exact constructions: bit for bit against the small frame's exact answer; the median also
      value for value against the tiled class on the same tall frame.  mid_atrous_moments with five layers has no exact
      construction: its float64 checker on the small frame, the small frame's bits on the tall one.
    * Sixteen rows per workgroup, h = 1 048 593, width 3, the one-thread-per-pixel kernels; each test's docstring says, from the
      dispatch code, what sends the call there.  The small frame is held to the filter's checker by its existing rule, the tall
      frame to the same reference through the period and, since these kernels sum in window order per pixel, to the bits of the
      GPU's own small-frame output.
    * The same two heights once through a tiled class, whose tiles_x * tiles_y sits in gridDim.x: mid_atrous_joint with one layer,
      and the tuned bilateral at radius 8.

Outputs hold NaN before each call and every plane lies between guard bands.  Each case prints its gridDim.y beside the device's
hipDeviceAttributeMaxGridDimY.
"""
import ctypes

import numpy as np
import pytest
import torch

import atrous_variance_inputs as avi
import image_denoising_filter_amd as mid
import guide_format_inputs as gi
import median_inputs as mi
import np_atrous_exact as ax
import np_atrous_variance_exact as vex
import np_bilateral_joint
import np_bilateral_temporal
import np_median
import np_nlm_joint
import np_nlm_layers
import np_nlm_layers_temporal
import np_temporal_accumulate_exact as tae
import oracle
import tall_inputs as ti
from conftest import rel_err
from tall_device import F32F32, F32U8, Plane, announce, dev, finish, max_grid_dim_y, planes_of, rows_on_device, table, wrong_rows

pytestmark = pytest.mark.gpu


# ---- four rows per workgroup ----------------------------------------------------------------------------------------------------------
def accumulate(ctx, t, h, w, clip):
    """mid_temporal_accumulate[_clip] over the planes t; returns (colour, state, variance) device tensors."""
    p = ti.ACCUM_PARAMS
    prm = mid.TemporalAccumParams(w, h, p["alpha"], p["alpha_moments"], p["history_max"], 4.0, F32U8)
    col, st, var = Plane((h, w, 4), torch.float32), Plane((h, w, 4), torch.float32), Plane((h, w), torch.float32)
    L = ti.ACCUM_LAYERS
    head = (ctx.handle, ctypes.byref(prm), (ctypes.c_float * 16)(*[tae.SIGMA] * L), t["frame"].ptr, table(t["layers"]), table(t["prev_layers"]), L,
            t["motion"].ptr, t["hist_colour"].ptr, t["hist_state"].ptr, None)
    torch.cuda.synchronize()
    if clip:
        rc = mid.lib.mid_temporal_accumulate_clip(*head, t["clip_lo"].ptr, t["clip_hi"].ptr, col.ptr, st.ptr, var.ptr, None)
    else:
        rc = mid.lib.mid_temporal_accumulate(*head, col.ptr, st.ptr, var.ptr, None)
    finish(ctx, rc, t, (col, st, var))
    return col.mid, st.mid, var.mid


@pytest.mark.parametrize("clip", (False, True), ids=("plain", "clip"))
@pytest.mark.parametrize("w", ti.WIDTHS)
def test_temporal_accumulate(ctx, w, clip):
    H, r = ti.H4, ti.ACCUM_REACH
    announce(f"temporal_accumulate{'_clip' if clip else ''} {w} wide", H, 4)
    pat = ti.accumulate_patterns(w)
    names = [n for n in pat if clip or not n.startswith("clip")]
    hs = ti.small_height(H, r)
    want = ti.accumulate_answer(ti.tiled(pat, hs), clip)
    small = accumulate(ctx, planes_of(pat, hs, names), hs, w, clip)
    for g, a in zip(small, want):
        assert np.array_equal(g.cpu().numpy().view(np.uint32), np.ascontiguousarray(a).view(np.uint32)), "the small frame against the exact answer"
    got = accumulate(ctx, planes_of(pat, H, names), H, w, clip)
    rows = rows_on_device(H, r, hs)
    for name, g, a in zip(("colour", "state", "variance"), got, want):
        assert not torch.isnan(g).any(), f"{name}: a pixel was not written"
        assert wrong_rows(g, dev(a), rows) == [], name


def atrous(ctx, t, h, w, L):
    prm = mid.AtrousParams(w, h, 0, 1, 0.0, F32F32)
    out = Plane((h, w, 4), torch.float32)
    torch.cuda.synchronize()
    rc = mid.lib.mid_atrous_joint(ctx.handle, ctypes.byref(prm), (ctypes.c_float * 16)(*[ax.SIGMA] * L), t["frame"].ptr, table(t["layers"]), L,
                                  out.ptr, mid.FMT_RGBA32F, None, None)
    finish(ctx, rc, t, (out,))
    return out.mid


@pytest.mark.parametrize("L", (5, 1), ids=("global-5-layers", "tiled-1-layer"))
@pytest.mark.parametrize("w", ti.WIDTHS)
def test_atrous_joint_one_pass(ctx, w, L):
    """Five layers: atrous_global_kernel (more than four layers: no LDS class, csrc/atrous.hip dispatch_atrous).  One layer: the tiled
    class of step 1, the same height with tiles_x * tiles_y in gridDim.x."""
    H, r = ti.H4, ti.ATROUS_REACH
    announce(f"atrous_joint {L} layers {w} wide", H, 4)
    pat = ti.atrous_patterns(w, L)
    hs = ti.small_height(H, r)
    want, share = ti.atrous_answer(ti.tiled(pat, hs))
    assert 0.02 < share < 0.98
    small = atrous(ctx, planes_of(pat, hs, pat), hs, w, L)
    assert np.array_equal(small.cpu().numpy().view(np.uint32), want.view(np.uint32)), "the small frame against the exact answer"
    got = atrous(ctx, planes_of(pat, H, pat), H, w, L)
    assert not torch.isnan(got).any(), "a pixel was not written"
    assert wrong_rows(got, dev(want), rows_on_device(H, r, hs)) == []


def frames_and_layers(t):
    """The frame planes and the flat layer table [frame][layer] of a three-frame set."""
    frames = [t[f"frame{f}"] for f in range(ti.TEMPORAL_FRAMES)]
    return frames, [p for f in range(ti.TEMPORAL_FRAMES) for p in t[f"layers{f}"]]


def variance_pass(ctx, t, h, w, L):
    prm = mid.AtrousVarianceParams(w, h, 0, 1, vex.SIGMA_LUM, vex.EPSILON, F32F32)
    out, vout = Plane((h, w, 4), torch.float32), Plane((h, w), torch.float32)
    torch.cuda.synchronize()
    rc = mid.lib.mid_atrous_variance(ctx.handle, ctypes.byref(prm), (ctypes.c_float * 16)(*[vex.SIGMA] * L), t["frame"].ptr, t["variance"].ptr,
                                     table(t["layers"]), L, out.ptr, mid.FMT_RGBA32F, vout.ptr, None, None)
    finish(ctx, rc, t, (out, vout))
    return out.mid, vout.mid


@pytest.mark.parametrize("w", ti.WIDTHS)
def test_atrous_variance_one_pass_global_class(ctx, w):
    """Five layers: variance_global_kernel (more than four layers: no comb class, csrc/atrous_variance.hip dispatch_variance)."""
    H, r, L = ti.H4, ti.ATROUS_REACH, 5
    announce(f"atrous_variance {L} layers {w} wide", H, 4)
    pat = ti.variance_patterns(w, L)
    hs = ti.small_height(H, r)
    want, share = ti.variance_answer(ti.tiled(pat, hs))
    assert 0.02 < share < 0.98
    small = variance_pass(ctx, planes_of(pat, hs, pat), hs, w, L)
    got = variance_pass(ctx, planes_of(pat, H, pat), H, w, L)
    rows = rows_on_device(H, r, hs)
    for name, s, g, a in zip(("colour", "variance"), small, got, want):
        assert np.array_equal(s.cpu().numpy().view(np.uint32), np.ascontiguousarray(a).view(np.uint32)), f"{name}: the small frame against the exact answer"
        assert not torch.isnan(g).any(), f"{name}: a pixel was not written"
        assert wrong_rows(g, dev(a), rows) == [], name


def temporal_pass(ctx, t, h, w, L):
    prm = mid.AtrousParams(w, h, 0, 1, 0.0, F32F32)
    out = Plane((h, w, 4), torch.float32)
    frames, layers = frames_and_layers(t)
    n = ti.TEMPORAL_FRAMES
    torch.cuda.synchronize()
    rc = mid.lib.mid_atrous_joint_temporal(ctx.handle, ctypes.byref(prm), (ctypes.c_float * 16)(*[ax.SIGMA] * L), table(frames, n), table(layers, n * L), L,
                                           n, ti.TEMPORAL_K, ti.TEMPORAL_T, 1, table([out], 1), mid.FMT_RGBA32F, None, None)
    finish(ctx, rc, t, (out,))
    return out.mid


@pytest.mark.parametrize("w", ti.WIDTHS)
def test_atrous_temporal_pass_global_class(ctx, w):
    """Five layers: atrous_temporal_global_kernel (more than four layers, csrc/atrous_temporal.hip dispatch_atrous_temporal); three
    frames, the middle output, one pass."""
    H, r, L = ti.H4, ti.ATROUS_REACH, 5
    announce(f"atrous_joint_temporal {L} layers {w} wide", H, 4)
    pat = ti.temporal_patterns(w, L)
    hs = ti.small_height(H, r)
    want, share = ti.temporal_answer(ti.tiled(pat, hs))
    assert 0.02 < share < 0.98
    small = temporal_pass(ctx, planes_of(pat, hs, pat), hs, w, L)
    assert np.array_equal(small.cpu().numpy().view(np.uint32), want.view(np.uint32)), "the small frame against the exact answer"
    got = temporal_pass(ctx, planes_of(pat, H, pat), H, w, L)
    assert not torch.isnan(got).any(), "a pixel was not written"
    assert wrong_rows(got, dev(want), rows_on_device(H, r, hs)) == []


def moments(ctx, t, h, w, L):
    prm = mid.AtrousMomentsParams(w, h, F32F32)
    out = Plane((h, w), torch.float32)
    frames, layers = frames_and_layers(t)
    n = ti.TEMPORAL_FRAMES
    torch.cuda.synchronize()
    rc = mid.lib.mid_atrous_moments(ctx.handle, ctypes.byref(prm), (ctypes.c_float * 16)(*avi.sigmas_of(L)), table(frames, n), table(layers, n * L), L,
                                    n, ti.TEMPORAL_K, ti.TEMPORAL_T, out.ptr, None)
    finish(ctx, rc, t, (out,))
    return out.mid


@pytest.mark.parametrize("w", ti.WIDTHS)
def test_atrous_moments_global_class(ctx, w):
    """Five layers: moments_global_kernel (more than four layers, csrc/atrous_variance.hip dispatch_moments).  No exact construction
    exists for the moments: the small frame is held to the float64 checker by the existing rule, |dV| <= 1e-5 max(1, M2), and the
    tall frame to the bits of the small one -- the kernel sums a pixel's taps in one order wherever the pixel lies."""
    H, r, L = ti.H4, ti.MOMENTS_REACH, 5
    announce(f"atrous_moments {L} layers {w} wide", H, 4)
    pat = ti.moments_patterns(w, L)
    hs = ti.small_height(H, r)
    ref, m2 = ti.moments_reference(ti.tiled(pat, hs), L)
    small = moments(ctx, planes_of(pat, hs, pat), hs, w, L)
    err = float(np.max(np.abs(small.cpu().numpy().astype(np.float64) - ref) / np.maximum(1.0, m2)))
    print(f"small frame {w} x {hs} against the float64 checker: {err:.3e}")
    assert err <= 1e-5
    got = moments(ctx, planes_of(pat, H, pat), H, w, L)
    assert not torch.isnan(got).any(), "a pixel was not written"
    assert wrong_rows(got, small, rows_on_device(H, r, hs)) == []


def median(ctx, frame, layers, h, w, radius):
    prm = mid.MedianParams(w, h, radius, F32F32)
    out = Plane((h, w, 4), torch.float32)
    L = len(layers)
    torch.cuda.synchronize()
    rc = mid.lib.mid_median_filter(ctx.handle, ctypes.byref(prm), (ctypes.c_float * 16)(*[mi.EXACT_SIGMA] * L), frame.ptr, table(layers), L,
                                   out.ptr, mid.FMT_RGBA32F, None)
    finish(ctx, rc, {"frame": frame, "layers": layers}, (out,))
    return out.mid


@pytest.mark.parametrize("radius", mi.RADII)
@pytest.mark.parametrize("w", ti.WIDTHS)
def test_median_global_class(ctx, w, radius):
    """Five layers -- the guide and four all-zero ones -- run median_global_kernel (more than four layers, csrc/median.hip
    launch_median); the guide alone runs the tiled class.  Weights are exactly 0 or 1, so both give the checker's values."""
    H = ti.H4
    announce(f"median radius {radius} {w} wide", H, 4)
    pat = ti.median_patterns(w)
    hs = ti.small_height(H, radius)
    fr = ti.tile_rows(pat["frame"], hs)
    gd = ti.tile_rows(pat["guide"], hs)
    want, _, exact = np_median.median(fr, [gd], [mi.EXACT_SIGMA], radius)
    assert exact.all()
    zero = np.zeros((ti.PERIOD, w, 4), np.float32)
    t = planes_of(dict(frame=pat["frame"], layers=[pat["guide"]] + [zero] * 4), H, ("frame", "layers"))
    got = median(ctx, t["frame"], t["layers"], H, w, radius)
    rows = rows_on_device(H, radius, hs)
    assert wrong_rows(got, dev(want), rows, values=True) == [], "the global class against the checker"
    assert not torch.isnan(got[..., 3]).any(), "a pixel was not written (alpha is copied, and finite)"
    tiled = median(ctx, t["frame"], t["layers"][:1], H, w, radius)
    ok = (got == tiled) | (torch.isnan(got) & torch.isnan(tiled))
    assert bool(ok.all()), "the global class against the tiled class on the same frame"


# ---- sixteen rows per workgroup -------------------------------------------------------------------------------------------------------
def bilateral(ctx, t, h, w, radius, layered):
    ss, sc = ti.BILATERAL_SIGMAS
    prm = mid.BilateralParams(w, h, ss, sc, radius, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)
    out = Plane((h, w, 4), torch.float32)
    torch.cuda.synchronize()
    if layered:
        rc = mid.lib.mid_bilateral_layers(ctx.handle, ctypes.byref(prm), t["frame"].ptr, table(t["layers"]), len(t["layers"]), out.ptr, None)
    else:
        rc = mid.lib.mid_bilateral(ctx.handle, ctypes.byref(prm), t["frame"].ptr, out.ptr, None)
    finish(ctx, rc, t, (out,))
    return out.mid


@pytest.mark.parametrize("layered", (True, False), ids=("layers-radius-18-generic", "plain-radius-8-tuned"))
def test_bilateral(ctx, layered):
    """The tuned kernel's sums depend on a pixel's place in its tile (rows per wave), and 37 and the tile height are coprime, so the
    tall frame of the tuned class is held to the oracle through the period, not to the small frame's bits; a wrapped row would hold
    another phase of a noisy pattern, far outside 1e-5.  Layered (mid_bilateral_layers) at radius 18: csrc/bilateral.hip, dispatch_radius, gives radii with a fixed-radius shape that
    shape and the others the run-time-radius tiled kernel while its tile fits the LDS; the two tiles of the layer modes do not fit
    above radius 17, which leaves bilateral_generic_kernel.  Plain at radius 8: the tuned tiled kernel, gridDim.x = tiles."""
    H, w = ti.H16, 3
    radius = ti.BILATERAL_GENERIC_RADIUS if layered else ti.BILATERAL_TUNED_RADIUS
    announce(f"bilateral{'_layers' if layered else ''} radius {radius}", H, 16)
    pat = ti.bilateral_patterns(w)
    names = ("frame", "layers") if layered else ("frame",)
    hs = ti.small_height(H, radius)
    t = ti.tiled(pat, hs)
    ss, sc = ti.BILATERAL_SIGMAS
    if layered:
        W = np.zeros((hs, w, 8), np.float32)
        for lay in t["layers"]:
            W = oracle.bilateral_layers_accum(t["frame"], lay, W, radius, ss, sc)
        ref = oracle.normalize(W)
    else:
        ref = oracle.bilateral_texture(t["frame"], radius, ss, sc)
    small = bilateral(ctx, planes_of(pat, hs, names), hs, w, radius, layered)
    err = rel_err(small.cpu().numpy(), ref)
    print(f"small frame {w} x {hs} against the oracle: {err:.3e}")
    assert err < 1e-5
    got = bilateral(ctx, planes_of(pat, H, names), H, w, radius, layered)
    assert not torch.isnan(got).any(), "a pixel was not written"
    rows = rows_on_device(H, radius, hs)
    err = float(((got - dev(ref).index_select(0, rows)).abs() / dev(ref).index_select(0, rows).abs().clamp(min=1.0)).max())
    print(f"tall frame {w} x {H} against the oracle through the period: {err:.3e}")
    assert err < 1e-5
    if layered:
        assert wrong_rows(got, small, rows) == [], "the bits of the GPU's own small frame"


def bilateral_joint(ctx, t, h, w):
    ss, sc = ti.BILATERAL_SIGMAS
    prm = mid.BilateralParams(w, h, ss, sc, ti.BILATERAL_JOINT_RADIUS, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)
    out = Plane((h, w, 4), torch.float32)
    L = len(t["layers"])
    torch.cuda.synchronize()
    rc = mid.lib.mid_bilateral_joint(ctx.handle, ctypes.byref(prm), None, table([t["frame"]], 1), table(t["layers"], L), L, 1, 0, 0, 1,
                                     table([out], 1), mid.FMT_RGBA32F, None)
    finish(ctx, rc, t, (out,))
    return out.mid


def held_to_checker_and_small_frame(what, small, got, ref, rows):
    """The existing rule of the bilateral family against the float64 checker on the small frame, the tall frame against the same
    reference through the period, and the bits of the GPU's own small frame."""
    err = rel_err(small.cpu().numpy(), ref)
    print(f"{what}: small frame against the float64 checker: {err:.3e}")
    assert err < gi.TOL
    assert not torch.isnan(got).any(), "a pixel was not written"
    want = dev(ref).index_select(0, rows)
    err = float(((got.double() - want).abs() / want.abs().clamp(min=1.0)).max())
    print(f"{what}: tall frame against the float64 checker through the period: {err:.3e}")
    assert err < gi.TOL
    assert wrong_rows(got, small, rows) == [], "the bits of the GPU's own small frame"


def test_bilateral_joint_generic(ctx):
    """Five layers at radius 1: more layers than the tiled kernels keep resident (kJointTiledLayers = 4) run
    bilateral_joint_generic_kernel at every radius (csrc/bilateral_joint.hip, launch_joint_tiled / dispatch_joint)."""
    H, w, r = ti.H16, 3, ti.BILATERAL_JOINT_RADIUS
    announce("bilateral_joint 5 layers radius 1", H, 16)
    pat = ti.bilateral_patterns(w, n_layers=ti.BILATERAL_JOINT_LAYERS)
    hs = ti.small_height(H, r)
    t = ti.tiled(pat, hs)
    ss, sc = ti.BILATERAL_SIGMAS
    (ref,) = np_bilateral_joint.bilateral_joint([t["frame"]], [t["layers"]], [sc] * ti.BILATERAL_JOINT_LAYERS, 0, r, ss)
    small = bilateral_joint(ctx, planes_of(pat, hs, pat), hs, w)
    got = bilateral_joint(ctx, planes_of(pat, H, pat), H, w)
    held_to_checker_and_small_frame("bilateral_joint", small, got, ref, rows_on_device(H, r, hs))


def bilateral_temporal(ctx, t, h, w, radius):
    ss, sc = ti.BILATERAL_SIGMAS
    prm = mid.BilateralParams(w, h, ss, sc, radius, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)
    out = Plane((h, w, 4), torch.float32)
    frames, layers = [t["frame0"], t["frame1"]], t["layers0"] + t["layers1"]
    torch.cuda.synchronize()
    rc = mid.lib.mid_bilateral_temporal(ctx.handle, ctypes.byref(prm), table(frames, 2), table(layers, len(layers)), len(t["layers0"]), 2, 1, 0, 1,
                                        table([out], 1), mid.FMT_RGBA32F, None)
    finish(ctx, rc, t, (out,))
    return out.mid


def test_bilateral_temporal_generic(ctx):
    """Two frames with two layers each at radius 18, output 0 with k = 1: the layered form's two tiles do not fit the LDS above
    radius 17, which leaves bilateral_pair_generic_kernel (csrc/bilateral_temporal.hip, dispatch_pair_radius)."""
    H, w, r = ti.H16, 3, ti.BILATERAL_GENERIC_RADIUS
    announce("bilateral_temporal 2 layers radius 18", H, 16)
    pat = ti.bilateral_pair_patterns(w)
    hs = ti.small_height(H, r)
    t = ti.tiled(pat, hs)
    ss, sc = ti.BILATERAL_SIGMAS
    (ref,) = np_bilateral_temporal.bilateral_temporal([t["frame0"], t["frame1"]], 1, r, ss, sc, layers=[t["layers0"], t["layers1"]], first=0, count=1)
    small = bilateral_temporal(ctx, planes_of(pat, hs, pat), hs, w, r)
    got = bilateral_temporal(ctx, planes_of(pat, H, pat), H, w, r)
    held_to_checker_and_small_frame("bilateral_temporal", small, got, np.asarray(ref), rows_on_device(H, r, hs))


NLM_SEARCH, NLM_PATCH, NLM_H, NLM_REACH = (-1, 2), (0, 2), 0.5, 2


def nlm_accum_normalize(ctx, t, h, w):
    prm = mid.NlmParams(w, h, NLM_H, NLM_SEARCH[0], NLM_SEARCH[1], NLM_PATCH[0], NLM_PATCH[1], mid.FMT_RGBA32F)
    W, out = Plane((h, w, 8), torch.float32), Plane((h, w, 4), torch.float32)
    W.mid.zero_()
    torch.cuda.synchronize()
    rc = mid.lib.mid_nlm_accum(ctx.handle, ctypes.byref(prm), t["frame"].ptr, t["frame"].ptr, W.ptr, None)
    assert rc == 0, mid.lib.mid_last_error()
    q = mid.NormalizeParams(w, h)
    rc = mid.lib.mid_normalize(ctx.handle, ctypes.byref(q), W.ptr, out.ptr, None)
    finish(ctx, rc, t, (W, out))
    return out.mid


def test_nlm_accum_generic_and_normalize(ctx):
    """Search [-1, 2), patch [0, 2): a patch range that is neither a tuned window nor one of the run-time strip kernel's patch ranges
    (csrc/nlm.hip dispatch_ranges, csrc/nlm_rt.hip, csrc/nlm_rt4.hip) is left to nlm_generic_kernel, here through mid_nlm_accum into a
    zeroed weight buffer, then mid_normalize.  The NLM rule: rel_err < 2e-5 against the oracle."""
    H, w, r = ti.H16, 3, NLM_REACH
    announce("nlm_accum search [-1, 2) patch [0, 2)", H, 16)
    pat = {"frame": ti.bilateral_patterns(w)["frame"]}
    hs = ti.small_height(H, r)
    fr = ti.tile_rows(pat["frame"], hs)
    ref = oracle.normalize(oracle.nlm_accum(fr, fr, np.zeros((hs, w, 8), np.float32), NLM_H, search=NLM_SEARCH, patch=NLM_PATCH))
    small = nlm_accum_normalize(ctx, planes_of(pat, hs, pat), hs, w)
    err = rel_err(small.cpu().numpy(), ref)
    print(f"nlm_accum + normalize: small frame against the oracle: {err:.3e}")
    assert err < 2e-5
    got = nlm_accum_normalize(ctx, planes_of(pat, H, pat), H, w)
    assert not torch.isnan(got).any(), "a pixel was not written"
    assert wrong_rows(got, small, rows_on_device(H, r, hs)) == [], "the bits of the GPU's own small frame"


def held_to_nlm_checker_and_small_frame(what, small, got, ref, rows):
    """The NLM rule (rel_err < 2e-5 against the float64 checker) on the small frame and, through the period, on the tall one, and
    the bits of the GPU's own small frame."""
    ref = np.asarray(ref, np.float64)
    err = rel_err(small.cpu().numpy(), ref)
    print(f"{what}: small frame against the float64 checker: {err:.3e}")
    assert err < 2e-5
    assert not torch.isnan(got).any(), "a pixel was not written"
    want = dev(ref).index_select(0, rows)
    err = float(((got.double() - want).abs() / want.abs().clamp(min=1.0)).max())
    print(f"{what}: tall frame against the float64 checker through the period: {err:.3e}")
    assert err < 2e-5
    assert wrong_rows(got, small, rows) == [], "the bits of the GPU's own small frame"


def nlm_params(w, h):
    return mid.NlmParams(w, h, NLM_H, NLM_SEARCH[0], NLM_SEARCH[1], NLM_PATCH[0], NLM_PATCH[1], mid.FMT_RGBA32F)


def nlm_layers(ctx, t, h, w):
    out = Plane((h, w, 4), torch.float32)
    prm = nlm_params(w, h)
    torch.cuda.synchronize()
    rc = mid.lib.mid_nlm_layers(ctx.handle, ctypes.byref(prm), t["frame0"].ptr, table(t["layers0"]), len(t["layers0"]), out.ptr, None)
    finish(ctx, rc, t, (out,))
    return out.mid


def test_nlm_layers_generic(ctx):
    """Search [-1, 2), patch [0, 2): csrc/nlm_layers.hip gives the two tuned windows (nlm_guide_for_window: 21x21 / 7x7 and
    14x14 / 6x6) to the strip kernel and every other window to nlm_layers_generic_kernel (launch_guide_per_pixel)."""
    H, w, r = ti.H16, 3, NLM_REACH
    announce("nlm_layers search [-1, 2) patch [0, 2)", H, 16)
    pat = {k: v for k, v in ti.bilateral_pair_patterns(w).items() if k.endswith("0")}
    hs = ti.small_height(H, r)
    t = ti.tiled(pat, hs)
    ref = np_nlm_layers.nlm_layers(t["frame0"], t["layers0"], NLM_H, NLM_SEARCH, NLM_PATCH)
    small = nlm_layers(ctx, planes_of(pat, hs, pat), hs, w)
    got = nlm_layers(ctx, planes_of(pat, H, pat), H, w)
    held_to_nlm_checker_and_small_frame("nlm_layers", small, got, ref, rows_on_device(H, r, hs))


def nlm_over_frames(ctx, t, h, w, joint):
    out = Plane((h, w, 4), torch.float32)
    prm = nlm_params(w, h)
    frames, layers = [t["frame0"], t["frame1"]], t["layers0"] + t["layers1"]
    L = len(t["layers0"])
    tail = (table(frames, 2), table(layers, len(layers)), L, 2, 1, 0, 1, table([out], 1), mid.FMT_RGBA32F, None)
    torch.cuda.synchronize()
    if joint:
        rc = mid.lib.mid_nlm_joint(ctx.handle, ctypes.byref(prm), (ctypes.c_float * 16)(*NLM_JOINT_HS), *tail)
    else:
        rc = mid.lib.mid_nlm_layers_temporal(ctx.handle, ctypes.byref(prm), *tail)
    finish(ctx, rc, t, (out,))
    return out.mid


NLM_JOINT_HS = (0.5, 0.8)


@pytest.mark.parametrize("joint", (False, True), ids=("nlm_layers_temporal", "nlm_joint"))
def test_nlm_over_frames_generic(ctx, joint):
    """Two frames with two layers each, output 0 with k = 1, search [-1, 2), patch [0, 2).  mid_nlm_layers_temporal:
    csrc/nlm_layers_temporal.hip dispatch_pair gives the two tuned windows to the strip kernel and every other window to
    nlm_layers_pair_generic_kernel.  mid_nlm_joint: csrc/nlm_joint.hip dispatch_joint does the same with nlm_joint_generic_kernel."""
    H, w, r = ti.H16, 3, NLM_REACH
    name = "nlm_joint" if joint else "nlm_layers_temporal"
    announce(f"{name} search [-1, 2) patch [0, 2)", H, 16)
    pat = ti.bilateral_pair_patterns(w)
    hs = ti.small_height(H, r)
    t = ti.tiled(pat, hs)
    frames, layers = [t["frame0"], t["frame1"]], [t["layers0"], t["layers1"]]
    if joint:
        (ref,) = np_nlm_joint.nlm_joint(frames, layers, list(NLM_JOINT_HS), 1, NLM_SEARCH, NLM_PATCH, first=0, count=1)
    else:
        (ref,) = np_nlm_layers_temporal.nlm_layers_temporal(frames, layers, 1, NLM_H, NLM_SEARCH, NLM_PATCH, first=0, count=1)
    small = nlm_over_frames(ctx, planes_of(pat, hs, pat), hs, w, joint)
    got = nlm_over_frames(ctx, planes_of(pat, H, pat), H, w, joint)
    held_to_nlm_checker_and_small_frame(name, small, got, ref, rows_on_device(H, r, hs))


def test_the_grid_limits_the_device_reports():
    """hipDeviceAttributeMaxGridDimX / Y / Z of device 0 (tall_device.max_grid_dim_y asserts that the three numbers are plausible
    grid limits, so a header with another numbering fails here and not inside a filter's test)."""
    y = max_grid_dim_y()
    print(f"hipDeviceAttributeMaxGridDimY = {y}; the tests here launch gridDim.y = {ti.GRID_Y}")
    assert y > 0
