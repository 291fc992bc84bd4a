"""CPU suite: layer-guided NLM (mid_nlm_layers_accum, mid_nlm_layers, mid_sequence_nlm_layers) is exported and bound, refuses a
NULL context before doing anything, and the CLI offers it as --modes nlm-layers and --animation-filter nlm-layers; the float64
checker of the GPU tests (np_nlm_layers.py) reduces to plain NLM and to the closed form of a constant guide."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import image_denoising_filter_amd as mid
import np_nlm_layers
import np_reference

CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
ARGC = {"mid_nlm_layers_accum": 6, "mid_nlm_layers": 7, "mid_sequence_nlm_layers": 10}


def test_entry_points_are_exported_and_bound():
    raw = ctypes.CDLL(mid.LIB_PATH)
    for name, argc in ARGC.items():
        assert hasattr(raw, name)
        assert name in mid.EXPORTED
        fn = getattr(mid.lib, name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == argc, name
    for m in ("nlm_layers_accum", "nlm_layers", "sequence_nlm_layers", "sequence_nlm_layers_pinned"):
        assert hasattr(mid.Context, m)


def test_null_context_is_refused_and_nothing_is_written():
    h, w = 8, 16
    img = np.ones((h, w, 4), np.float32)
    lyr = np.zeros((h, w, 4), np.uint8)
    out = np.full((h, w, 4), 7, np.uint8)
    W = np.full((h, w, 8), 3.0, np.float32)
    p = mid.NlmParams(w, h, 0.5, -7, 7, -3, 3, mid.FMT_RGBA32F)
    lt = (ctypes.c_void_p * 1)(lyr.ctypes.data)
    assert mid.lib.mid_nlm_layers_accum(None, ctypes.byref(p), img.ctypes.data, lyr.ctypes.data, W.ctypes.data, None) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    assert mid.lib.mid_nlm_layers(None, ctypes.byref(p), img.ctypes.data, lt, 1, out.ctypes.data, None) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    fr = (ctypes.c_void_p * 1)(img.ctypes.data)
    ou = (ctypes.c_void_p * 1)(out.ctypes.data)
    t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    assert mid.lib.mid_sequence_nlm_layers(None, ctypes.byref(p), fr, 1, lt, 1, ou, mid.FMT_RGBA8, 1, t) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    assert (out == 7).all() and (W == 3.0).all() and list(t) == [-1.0, -1.0, -1.0]


def test_cli_help_lists_nlm_layers_for_modes_and_animation_filter():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    modes = r.stdout.split("--modes", 1)[1].split("--gpu-only", 1)[0]
    assert "nlm-layers" in modes and "output-nonlinear-nlm-layers" in modes
    anim = r.stdout.split("--animation-filter", 1)[1].split("--gpus", 1)[0]
    assert "nlm-layers" in anim and "output-animation-nonlinear-nlm-layers" in anim


@pytest.mark.parametrize("search,patch", [((-7, 7), (-3, 3)), ((-3, 4), (-1, 2)), ((-2, 3), (-1, 3)), ((-4, 5), (0, 1))])
def test_checker_with_the_input_as_guide_is_plain_nlm(search, patch):
    rng = np.random.default_rng(5)
    h, w = 13, 17
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 9, yy * 11, (xx + yy) * 5, np.full_like(xx, 255)], -1) + rng.integers(0, 6, (h, w, 4))
    img = np.clip(base, 0, 255).astype(np.uint8)
    num, den = np_nlm_layers.nlm_layers_sums(img, [img], 0.5, search, patch)
    f = img.astype(np.float64) / 255.0
    rn, rd = np_reference.nlm_sums(f, f, 0.5, search, patch)
    assert np.abs(num - rn).max() <= 1e-12 * max(1.0, np.abs(rn).max())
    assert np.abs(den - rd).max() <= 1e-12 * max(1.0, np.abs(rd).max())


def test_checker_on_a_constant_guide_is_the_box_mean():
    # a constant guide gives every offset whose patch stays inside the image the weight exp(0) = 1, so an interior pixel is
    # sum of the input over its search window / (S^2 + 0.001), whatever the input
    rng = np.random.default_rng(6)
    h, w = 31, 33
    search, patch = (-7, 7), (-3, 3)
    img = rng.random((h, w, 4)).astype(np.float32)
    guide = np.full((h, w, 4), 140, np.uint8)
    out = np_nlm_layers.nlm_layers(img, [guide], 0.5, search, patch)
    S = search[1] - search[0]
    m = max(-search[0], search[1]) + max(-patch[0], patch[1])
    for y in range(m, h - m):
        for x in range(m, w - m):
            win = img[y + search[0]:y + search[1], x + search[0]:x + search[1]].astype(np.float64)
            assert np.allclose(out[y, x], win.sum((0, 1)) / (S * S + 0.001), rtol=1e-12, atol=0)


def test_checker_without_layers_is_magenta():
    img = np.zeros((4, 5, 4), np.float32)
    out = np_nlm_layers.nlm_layers(img, [], 0.5, (-7, 7), (-3, 3))
    assert (out == np.array([1.0, 0.0, 1.0, 1.0])).all()
