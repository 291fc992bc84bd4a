"""CPU suite: the bilateral over neighbouring frames (mid_bilateral_pair_accum, mid_bilateral_layers_pair_accum,
mid_bilateral_temporal, mid_sequence_bilateral_temporal) is exported and bound as the header declares it, refuses a NULL context
before doing anything, and the CLI offers it as --animation-filter bilateral-temporal / layers-temporal; the float64 checker of
the GPU tests (np_bilateral_temporal.py) reproduces three answers that need no kernel."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import image_denoising_filter_amd as mid
import f64_checker
import np_bilateral_temporal as chk

CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
ARGC = {"mid_bilateral_pair_accum": 6, "mid_bilateral_layers_pair_accum": 7, "mid_bilateral_temporal": 12,
        "mid_sequence_bilateral_temporal": 13}
RTOL = 1e-12                      # the project's bound for its float64 checkers
CPU = torch.device("cpu")


def _close(a, b):
    return np.abs(a - b).max() <= RTOL * max(1.0, np.abs(b).max())


def test_entry_points_are_exported_and_bound_as_declared():
    raw = ctypes.CDLL(mid.LIB_PATH)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi_denoise.h")).read(), flags=re.S)
    for name, argc in ARGC.items():
        assert hasattr(raw, name)
        assert name in mid.EXPORTED
        fn = getattr(mid.lib, name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == argc, name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert decl, f"{name} is not declared in mi_denoise.h"
        params = [a.strip() for a in decl.group(1).split(",")]
        assert len(params) == argc, (name, params)
        for a, t in zip(params, fn.argtypes):           # an int parameter is bound as c_int, a pointer as a pointer type
            assert (("*" not in a) and a.startswith("int ")) == (t is ctypes.c_int), (name, a, t)
    for m in ("bilateral_pair_accum", "bilateral_layers_pair_accum", "bilateral_temporal", "sequence_bilateral_temporal",
              "sequence_bilateral_temporal_pinned"):
        assert hasattr(mid.Context, m)


def test_null_context_is_refused_and_nothing_is_written():
    h, w = 8, 16
    img = np.ones((h, w, 4), np.float32)
    lyr = np.zeros((h, w, 4), np.uint8)
    out = np.full((h, w, 4), 7, np.uint8)
    W = np.full((h, w, 8), 3.0, np.float32)
    p = mid.BilateralParams(w, h, 2.0, 0.2, 4, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)
    fr = (ctypes.c_void_p * 1)(img.ctypes.data)
    lt = (ctypes.c_void_p * 1)(lyr.ctypes.data)
    ou = (ctypes.c_void_p * 1)(out.ctypes.data)
    assert mid.lib.mid_bilateral_pair_accum(None, ctypes.byref(p), img.ctypes.data, img.ctypes.data, W.ctypes.data, None) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    assert mid.lib.mid_bilateral_layers_pair_accum(None, ctypes.byref(p), lyr.ctypes.data, lyr.ctypes.data, img.ctypes.data,
                                                   W.ctypes.data, None) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    assert mid.lib.mid_bilateral_temporal(None, ctypes.byref(p), fr, lt, 1, 1, 0, 0, 1, ou, mid.FMT_RGBA8, None) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    assert mid.lib.mid_sequence_bilateral_temporal(None, ctypes.byref(p), fr, 1, lt, 1, 0, 0, 1, ou, mid.FMT_RGBA8, 1, t) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    assert (out == 7).all() and (W == 3.0).all() and list(t) == [-1.0, -1.0, -1.0]


def test_cli_offers_both_filters(tmp_path):
    frame = np.full((4, 8, 4), 200, np.uint8)
    for i in range(2):      # (the PNG codec is host code: two tiny frames for the refusal that comes after frame discovery)
        assert mid.lib.mid_image_save(str(tmp_path / f"f_{i:04d}.png").encode(), frame.ctypes.data, 8, 4, mid.FMT_RGBA8) == 0
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    anim = r.stdout.split("--animation-filter", 1)[1].split("--gpus", 1)[0]
    assert "bilateral-temporal" in anim and re.search(r"(?<![-\w])layers-temporal", anim) and "--temporal-k" in anim
    assert "output-animation-nonlinear-bialteral-multiframe" in anim and "output-animation-nonlinear-bialteral-layers-multiframe" in anim
    for value in ("bilateral-temporal", "layers-temporal"):
        # the value is accepted (the run then stops at the missing file, not at the option) ...
        r = subprocess.run([CLI, "/nonexistent/f_0000.png", "--animation", "--animation-filter", value],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "unknown --animation-filter" not in r.stdout + r.stderr
        # ... needs --animation ...
        r = subprocess.run([CLI, "/nonexistent/f_0000.png", "--animation-filter", value], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--animation" in r.stdout + r.stderr
        # ... and has no RCCL halo exchange
        r = subprocess.run([CLI, str(tmp_path / "f_0000.png"), "--animation", "--animation-filter", value, "--halo", "rccl", "--gpu-only",
                            "--outdir", str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--halo rccl is not available with --animation-filter " + value in r.stdout + r.stderr
        assert not list(tmp_path.glob("output-*"))
    r = subprocess.run([CLI, "/nonexistent/f_0000.png", "--animation", "--animation-filter", "bilateral-temporalx"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "unknown --animation-filter" in r.stdout + r.stderr
    m = re.search(r"unknown --animation-filter[^\n]*", r.stdout + r.stderr).group(0)
    assert "bilateral-temporal" in m.replace("bilateral-temporalx", "") and "layers-temporal" in m


def _frames(rng, n, h, w):
    return [rng.random((h, w, 4)).astype(np.float32) for _ in range(n)]


def _guides(rng, L, h, w, shift=0):
    yy, xx = np.mgrid[0:h, 0:w]
    return [np.clip(np.stack([xx * 9 + i + shift, yy * 11, (xx + yy) * 5, np.full_like(xx, 255)], -1) + rng.integers(0, 6, (h, w, 4)), 0, 255)
            .astype(np.uint8) for i in range(L)]


def _single(frame, guides, R, ss, sc):
    """(num, den) of the single-frame filter by f64_checker: the sum over the guides of bilateral_sums(frame, guide)."""
    num = den = 0
    for g in guides:
        a, b = f64_checker.bilateral_sums(frame, chk.decode(g), R, ss, sc, dev=CPU)
        num, den = num + a.numpy(), den + b.numpy()
    return num, den


@pytest.mark.parametrize("layered", [False, True])
def test_known_answer_a_k0_is_the_single_frame_filter(layered):
    rng = np.random.default_rng(61)
    h, w, n, R = 13, 19, 3, 3
    frames = _frames(rng, n, h, w)
    layers = [_guides(rng, 2, h, w, 3 * f) for f in range(n)] if layered else None
    got = chk.bilateral_temporal(frames, 0, R, 2.0, 0.2, layers=layers, dev=CPU)
    assert len(got) == n
    for t in range(n):
        num, den = _single(frames[t], layers[t] if layered else [frames[t]], R, 2.0, 0.2)
        assert _close(got[t], num / den[..., None]), t
    sub = chk.bilateral_temporal(frames, 0, R, 2.0, 0.2, layers=layers, first=1, count=1, dev=CPU)
    assert len(sub) == 1 and np.array_equal(sub[0], got[1])


@pytest.mark.parametrize("k", [1, 2])
def test_known_answer_b_equal_guides_give_the_mean_of_the_single_frame_results(k):
    # with the guides equal across frames every neighbour's weights -- and so its denominator -- are those of the single-frame
    # layered filter of that neighbour: sum_f num_f / (m den) = mean_f (num_f / den)
    rng = np.random.default_rng(62)
    h, w, n, R = 13, 19, 4, 3
    frames, guides = _frames(rng, n, h, w), _guides(rng, 2, h, w)
    got = chk.bilateral_temporal(frames, k, R, 2.0, 0.2, layers=[guides] * n, dev=CPU)
    singles = []
    for f in range(n):
        num, den = _single(frames[f], guides, R, 2.0, 0.2)
        singles.append(num / den[..., None])
    for t in range(n):
        win = chk.window(n, t, k)
        assert _close(got[t], sum(singles[f] for f in win) / len(win)), t


def test_known_answer_c_a_mismatching_neighbour_is_switched_off():
    # frames 0 and 1 have guides of byte 255, frame 2 of byte 0: |dG|^2 = 3 at every tap of frame 2 -- its out-of-image texels,
    # which are 0 as well, included -- and at colorSigma 0.2 its every weight carries exp(-0.5 * 3 / 0.04) = e^-37.5 = 5e-17
    # beside the centre weight 1 of the target's own frame: below the bound
    assert np.exp(-37.5) < 1e-16
    rng = np.random.default_rng(63)
    h, w, n, k, R = 13, 19, 3, 1, 3
    frames = _frames(rng, n, h, w)
    zero, full = np.zeros((h, w, 4), np.uint8), np.full((h, w, 4), 255, np.uint8)
    layers = [[full], [full], [zero]]
    got = chk.bilateral_temporal(frames, k, R, 2.0, 0.2, layers=layers, dev=CPU)
    without = chk.bilateral_temporal(frames, k, R, 2.0, 0.2, layers=layers, skip=(2,), first=0, count=2, dev=CPU)
    assert _close(got[0], without[0])                      # (frame 2 is outside frame 0's window anyway)
    assert _close(got[1], without[1])                      # frame 2 switched off, at every pixel
    # for frame 2 (target byte 0) frame 1 is switched off only where its window stays inside the image: an out-of-image texel
    # of frame 1 is 0 and matches
    alone = chk.bilateral_temporal(frames, 0, R, 2.0, 0.2, layers=layers, first=2, count=1, dev=CPU)
    assert _close(got[2][R:-R, R:-R], alone[0][R:-R, R:-R]) and not _close(got[2], alone[0])
    # and the switched-off neighbour is not simply ignored by the checker: with matching guides it does change the output
    match = chk.bilateral_temporal(frames, k, R, 2.0, 0.2, layers=[[full]] * 3, first=1, count=1, dev=CPU)
    assert not _close(match[0], without[1])
