"""CPU suite: history clipping (include/mi_denoise.h, section a4m) is present in every layer, its Python keywords are checked before
any GPU work, the GPU tests' input recipe (tests/history_clip_inputs.py) does to the checkers what the tests rely on, and the two
numbers of the sequence test's demonstration follow from the checkers.

The conditions on the recipe, on 261 x 131, for every motion field and L the GPU tests use, both radii and both gammas: among the
pixels whose history has a weight (S > 0) at least a fifth have a channel clipped and at least a fifth have none clipped.  They are
conditions on the INPUTS, not tolerances; the measured shares stand in the recipe's docstring.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import history_clip_inputs as hci
import image_denoising_filter_amd as mid
from np_color_bounds import color_bounds
from np_temporal_accumulate_clip import temporal_accumulate_clip as check

NEW = ("mid_color_bounds", "mid_temporal_accumulate_clip", "mid_sequence_atrous_recursive_clip")


def test_header_library_and_table_carry_the_new_entry_points():
    src = open(os.path.join(ROOT, "include", "mi_denoise.h")).read()
    assert "a4m" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(mid.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in mi_denoise.h"
        assert hasattr(raw, name), f"{name} is not exported by libmi_denoise.so"
        assert name in mid.EXPORTED
    assert re.search(r"typedef struct mid_color_bounds_params \{\s*int32_t width, height;\s*int32_t radius;\s*float\s+gamma;\s*int32_t format;\s*\} mid_color_bounds_params;", code)
    P = mid.ColorBoundsParams
    assert (P.width.offset, P.height.offset, P.radius.offset, P.gamma.offset, P.format.offset, ctypes.sizeof(P)) == (0, 4, 8, 12, 16, 20)
    assert "ColorBoundsParams" in mid.__all__


def test_the_python_layer_has_the_keywords_and_their_defaults():
    sig = inspect.signature(mid.Context.color_bounds).parameters
    assert list(sig) == ["self", "frame", "radius", "gamma"] and [sig[k].default for k in ("radius", "gamma")] == [1, 1.0]
    sig = inspect.signature(mid.Context.temporal_accumulate).parameters
    assert list(sig)[-2:] == ["clip_lo", "clip_hi"] and sig["clip_lo"].default is None and sig["clip_hi"].default is None
    for fn in (mid.Context.sequence_atrous_recursive, mid.Context.sequence_atrous_recursive_pinned):
        sig = inspect.signature(fn).parameters
        assert list(sig)[-2:] == ["clip_gamma", "clip_radius"] and sig["clip_gamma"].default is None and sig["clip_radius"].default == 1


def test_out_of_range_keywords_raise_before_any_gpu_work():
    """The methods are called without a context (self = None): a ValueError must come before anything touches it."""
    frame = np.zeros((4, 5, 4), np.float32)
    for kw in (dict(radius=0), dict(radius=3), dict(radius=1.5), dict(radius=True), dict(gamma=-0.5), dict(gamma=float("nan")), dict(gamma=float("inf")),
               dict(gamma=1e39), dict(gamma=None)):
        with pytest.raises(ValueError, match="clip"):
            mid.Context.color_bounds(None, frame, **kw)
    layers = [[np.zeros((4, 5, 4), np.uint8)]]
    for kw in (dict(clip_radius=2), dict(clip_gamma=1.0, clip_radius=3), dict(clip_gamma=1.0, clip_radius=0), dict(clip_gamma=-1.0),
               dict(clip_gamma=float("nan")), dict(clip_gamma=float("inf"))):
        with pytest.raises(ValueError, match="clip"):
            mid.Context.sequence_atrous_recursive(None, [frame], layers, [0.1], **kw)
        with pytest.raises(ValueError, match="clip"):
            mid.Context.sequence_atrous_recursive_pinned(None, [0], [0], 5, 4, 0, [0], 1, [0.1], **kw)
    plane = np.zeros((4, 5, 4), np.float32)
    for kw in (dict(clip_lo=plane), dict(clip_hi=plane)):
        with pytest.raises(ValueError, match="both or neither"):
            mid.Context.temporal_accumulate(None, frame, [], None, [], **kw)


def test_help_lists_the_options():
    cli = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
    h = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("--history-clip GAMMA", "--history-clip-radius R"):
        assert opt in h, opt
    assert "--history-clip, --history-clip-radius;" in h                     # and the atrous-recursive paragraph names them


@pytest.mark.parametrize("radius", (1, 2))
@pytest.mark.parametrize("gamma", hci.GAMMAS)
def test_the_recipe_meets_its_conditions(gamma, radius):
    for fdt in (np.float32, np.uint8):
        shares = []
        for motion in hci.MOTIONS:
            for L in hci.LAYERS:
                args, kw = hci.case(hci.SHAPE, L, fdt, np.uint8, motion, False, 0)
                lo, hi = hci.boxes_of(args[0], radius, gamma)
                out = check(*args, **kw, clip_lo=lo, clip_hi=hi)
                pos = out["S"] > 0
                clipped = float(out["clipped"].any(-1)[pos].mean())
                shares.append(clipped)
                assert pos.mean() > 0.5 and clipped >= 0.2 and 1 - clipped >= 0.2, (np.dtype(fdt).name, gamma, radius, motion, L, clipped)
        print(f"{np.dtype(fdt).name} gamma {gamma} radius {radius}: a channel clipped on {min(shares):.3f} .. {max(shares):.3f} of the pixels with S > 0")


def test_the_demonstration_follows_from_the_checkers():
    """The accumulation chain of the demonstration with the checkers alone (feedback 0, zero motion, one constant layer; the a-trous
    pass of a locally constant plane is that plane): at the square's centre, on the frame of the switch, the clipped history is
    replaced -- the box of a constant neighbourhood is [B, B] -- and the unclipped one keeps 0.8 of the step."""
    frames, layers = hci.demo_frames()
    A, B, t6 = hci.DEMO_A, hci.DEMO_B, hci.DEMO_SWITCH
    y, x = hci.DEMO_CENTRE
    for clip in (True, False):
        hist = None
        for t in range(t6 + 1):
            kw = dict(hist=hist, alpha=0.2, alpha_moments=0.2, history_max=32, history_full=4)
            if clip and hist is not None:
                lo, hi = hci.boxes_of(frames[t], 1, 1.0)
                if t == t6:
                    assert np.array_equal(lo[y, x, :3], np.float32([B] * 3)) and np.array_equal(hi[y, x], lo[y, x]) and lo[y, x, 3] == 9
                kw.update(clip_lo=lo, clip_hi=hi)
            out = check(frames[t], layers[t], layers[t - 1] if t else layers[t], [0.1], **kw)
            hist = (out["colour"], out["state"])
            if t == t6 - 1:
                assert np.allclose(out["colour"][y, x, :3], A, rtol=1e-7) and out["state"][y, x, 2] == t6
        c = out["colour"][y, x, :3]
        assert out["state"][y, x, 2] == t6 + 1 >= 5                          # N' = 7: 1 / N' < alpha, the factor is alpha
        want = B if clip else A + float(np.float32(0.2)) * (B - A)
        assert np.abs(c - want).max() <= 1e-7, (clip, c, want)
    assert abs((A + 0.2 * (B - A)) - B) > 0.3                                 # the ghost the clip removes: 0.8 of the step
