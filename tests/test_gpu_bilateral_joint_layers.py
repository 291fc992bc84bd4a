"""GPU suite: every layer slot of the joint bilateral live, and float64 parity at L = 2, L = 4 and on both sides of every boundary of
the (radius, L) -> class table (include/mi_denoise.h, section a4e; restated in opaque_vote_cases.joint_class and held
against both by tests/test_bilateral_joint_classes.py).

tests/test_gpu_bilateral_joint.py holds slots 1..3 with all-zero layers or at exactly L = 3.  A zero layer says nothing about the
slot it sits in: centre 0 - tile 0 = 0 whatever plane, scl[l] or centre register is read.  Here:

  B1  tiled kernels, ONE live layer G in slot l of L = 2, 3, 4 (all-zero layers elsewhere, arbitrary sigmas there): the bits of L = 1
      with [G] -- a zero layer contributes fma(-0, 0, arg) = arg wherever it sits in the chain.  Pins fill_planes (slots >= 1) against
      the fused fill_colour_and_planes (slot 0), every plane offset, scl[l] and the centre registers of every slot.
  B2  per pixel (r = 8 at L = 5 and 16): moving the live layer between slots changes no bit (fmaf(0, kc, arg) = arg), and each result
      is within 1e-5 of the tiled L = 1 result.
  B3  two live layers swapped together with their sigmas: within 1e-5 (the chain's order differs, so the bits may).
  C   np_bilateral_joint on guide_format_inputs' HDR frames and render layers, every pixel of every output, tolerance gi.TOL = 1e-5
      under the header's condition |g| <= 16 sigma_l, which each test asserts first: tuned r = 4 and 8 at L = 2 and 4 (r = 8, L = 4 is
      the launch with exactly 160 KB of LDS); the run-time-radius kernel at its largest tile per layer count, (r 14, L 2) 161,920 B,
      (r 9, L 3), (r 7, L 4); the per-pixel kernel just across each boundary, (r 10, L 2), (r 15, L 2), (r 14, L 3), (r 9, L 4).
"""
import numpy as np
import pytest

import guide_format_inputs as gi
import np_bilateral_joint as chk
import opaque_vote_cases as ov
from conftest import rel_err
from test_gpu_bilateral_joint import DTYPES, N, frames_of, guides_of, same

pytestmark = pytest.mark.gpu

WORST = {}                                             # class -> worst error against float64, printed by the last test of the file
OTHER_SIGMAS = (0.01, 3.0, 0.3, 0.07)                  # of the all-zero layers: anything


def ids_dt(d):
    return np.dtype(d).name


# ---- B1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gdt", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("r,shape", [(4, (20, 70)), (4, (33, 130)), (8, (20, 70)), (8, (33, 130)), (3, (20, 70)), (7, (20, 70))],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"r{v}")
def test_one_live_layer_in_any_slot_has_the_bits_of_one_layer(ctx, r, shape, gdt):
    fr = frames_of(shape, np.float32)
    gl, s = guides_of(shape, gdt)
    zero = np.zeros(shape + (4,), gdt)
    kw = dict(radius=r, sigma_s=gi.SIGMA_S)
    want = ctx.bilateral_joint(fr, gl, [s], 1, **kw)
    for L in (2, 3, 4):
        assert ov.joint_class(r, L) == ("tuned" if r in ov.BIL_SHAPES else "run-time radius")
        for l in range(L):
            layers = [[zero] * l + ls + [zero] * (L - 1 - l) for ls in gl]
            sig = list(OTHER_SIGMAS[:L])
            sig[l] = s
            got = ctx.bilateral_joint(fr, layers, sig, 1, **kw)
            assert len(got) == N and all(same(g, x) for g, x in zip(got, want)), f"live layer in slot {l} of {L}"


# ---- B2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gdt", DTYPES, ids=ids_dt)
@pytest.mark.parametrize("L", [5, 16])
def test_one_live_layer_per_pixel_in_any_slot(ctx, L, gdt):
    shape, r = (12, 40), 8
    assert ov.joint_class(r, L) == "per pixel" and ov.joint_class(r, 1) == "tuned"
    fr = frames_of(shape, np.float32)
    gl, s = guides_of(shape, gdt)
    zero = np.zeros(shape + (4,), gdt)
    kw = dict(radius=r, sigma_s=gi.SIGMA_S)
    tiled = ctx.bilateral_joint(fr, gl, [s], 1, **kw)
    first = None
    for l in sorted({0, 1, 4, L - 1}):
        sig = [OTHER_SIGMAS[i % 4] for i in range(L)]
        sig[l] = s
        got = ctx.bilateral_joint(fr, [[zero] * l + ls + [zero] * (L - 1 - l) for ls in gl], sig, 1, **kw)
        first = got if first is None else first
        assert all(same(g, x) for g, x in zip(got, first)), f"slot {l} against slot 0"
        err = max(rel_err(g, x) for g, x in zip(got, tiled))
        print(f"per pixel r=8 L={L} live slot {l} against tiled L=1, {np.dtype(gdt).name} guides: {err:.3e}")
        assert err < gi.TOL


# ---- B3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gdt", [np.uint8, np.float32], ids=ids_dt)
@pytest.mark.parametrize("r,L", [(4, 2), (8, 2), (8, 4), (3, 2), (8, 5)], ids=lambda v: str(v))
def test_two_live_layers_swapped_with_their_sigmas(ctx, r, L, gdt):
    shape = (20, 70)
    fr = frames_of(shape, np.float32)
    gl, s = guides_of(shape, gdt, 2)
    sa, sb = s, 2.0 * s
    zero = np.zeros(shape + (4,), gdt)
    pad, psig = [zero] * (L - 2), list(OTHER_SIGMAS[:L - 2])
    kw = dict(radius=r, sigma_s=gi.SIGMA_S)
    ab = ctx.bilateral_joint(fr, [[ls[0], ls[1]] + pad for ls in gl], [sa, sb] + psig, 1, **kw)
    ba = ctx.bilateral_joint(fr, [[ls[1], ls[0]] + pad for ls in gl], [sb, sa] + psig, 1, **kw)
    err = max(rel_err(x, y) for x, y in zip(ab, ba))
    print(f"{ov.joint_class(r, L)} r={r} L={L} {np.dtype(gdt).name}: layers swapped {err:.3e}")
    assert err < gi.TOL
    one = ctx.bilateral_joint(fr, [[ls[0]] for ls in gl], [sa], 1, **kw)
    assert max(rel_err(x, y) for x, y in zip(ab, one)) > 100 * gi.TOL, "the second layer matters"


# ---- C -------------------------------------------------------------------------------------------------------------------------------
def layer_set(shape, L, gdt):
    """([frame][layer] guides, sigmas): L = 2 normals and depth; L = 3 the three render layers; L = 4 those and a second seed's albedo."""
    base = gi.render_layers(shape, N, gdt)
    if L == 2:
        return [[ls[0], ls[2]] for ls in base], (0.25, 0.5)
    if L == 3:
        return base, (1.0, 2.0, 0.5)
    other = gi.render_layers(shape, N, gdt, seed=57)
    return [ls + [os_[1]] for ls, os_ in zip(base, other)], (1.0, 2.0, 0.5, 1.0)


def parity(ctx, cls, r, L, gdt, runs):
    assert ov.joint_class(r, L) == cls
    worst = 0.0
    for shape, ks in runs:
        fr = gi.hdr_frames(shape, N, translucent=True)
        gl, sig = layer_set(shape, L, gdt)
        assert len(sig) == L and all(gi.max_guide_ratio([[ls[l]] for ls in gl], sig[l]) <= 16.0 for l in range(L))
        for k in ks:
            got = ctx.bilateral_joint(fr, gl, list(sig), k, radius=r, sigma_s=gi.SIGMA_S)
            want = chk.bilateral_joint(fr, gl, sig, k, r, gi.SIGMA_S)
            assert len(got) == len(want) == N
            err = max(rel_err(g, x) for g, x in zip(got, want))           # every pixel of every output
            print(f"{cls} r={r} L={L} {np.dtype(gdt).name} guides {shape} k={k}: worst rel err against float64 {err:.3e}")
            worst = max(worst, err)
    WORST[cls] = max(WORST.get(cls, 0.0), worst)
    return worst


BOTH = (((17, 65), (0, 2)), ((20, 70), (1,)))
ONE = (((20, 70), (1,)),)                              # radii >= 14: the float64 checker stays at a few seconds


@pytest.mark.parametrize("gdt", [np.float32, np.float16], ids=ids_dt)
@pytest.mark.parametrize("L", [2, 4])
@pytest.mark.parametrize("r", [4, 8])
def test_tuned_kernels_match_the_float64_checker_at_two_and_four_layers(ctx, r, L, gdt):
    assert parity(ctx, "tuned", r, L, gdt, BOTH) < gi.TOL


@pytest.mark.parametrize("r,L", [(14, 2), (9, 3), (7, 4)], ids=lambda v: str(v))
def test_run_time_radius_kernel_matches_the_float64_checker_at_its_largest_tiles(ctx, r, L):
    assert ov.joint_class(r + 1, L) == "per pixel" or r + 1 == 8
    assert parity(ctx, "run-time radius", r, L, np.float32, ONE if r >= 14 else BOTH) < gi.TOL


@pytest.mark.parametrize("r,L", [(10, 2), (15, 2), (14, 3), (9, 4)], ids=lambda v: str(v))
def test_per_pixel_kernel_matches_the_float64_checker_across_each_boundary(ctx, r, L):
    assert ov.joint_class(r - 1, L) != "per pixel" or ov.joint_class(r, L - 1) != "per pixel"      # one radius, or one layer, less is tiled
    assert parity(ctx, "per pixel", r, L, np.float32, ONE if r >= 14 else BOTH) < gi.TOL


def test_report_worst_errors():
    """Not a check: prints the figures DESIGN 3.8 quotes (run with -s)."""
    for cls, err in sorted(WORST.items()):
        print(f"{err:.3e}  {cls}")
