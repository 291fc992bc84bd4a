"""CPU suite: the whole-animation bilateral entry point (mid_sequence_bilateral) is exported and bound, refuses a NULL
context before doing anything, and the CLI offers it as --animation-filter."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import ROOT

import image_denoising_filter_amd as mid

CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")


def test_sequence_bilateral_is_exported_and_bound():
    raw = ctypes.CDLL(mid.LIB_PATH)
    assert hasattr(raw, "mid_sequence_bilateral")
    assert "mid_sequence_bilateral" in mid.EXPORTED
    assert mid.lib.mid_sequence_bilateral.restype is ctypes.c_int
    assert len(mid.lib.mid_sequence_bilateral.argtypes) == 10
    assert hasattr(mid.Context, "sequence_bilateral") and hasattr(mid.Context, "sequence_bilateral_pinned")


def test_null_context_is_refused_and_nothing_is_written():
    h, w = 8, 16
    frame = np.ones((h, w, 4), np.float32)
    out = np.full((h, w, 4), 7, np.uint8)
    p = mid.BilateralParams(w, h, 2.0, 0.2, 8, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)
    fr = (ctypes.c_void_p * 1)(frame.ctypes.data)
    ou = (ctypes.c_void_p * 1)(out.ctypes.data)
    t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    for layers, n_layers in ((None, 0), ((ctypes.c_void_p * 1)(out.ctypes.data + 0), 1)):
        rc = mid.lib.mid_sequence_bilateral(None, ctypes.byref(p), fr, 1, layers, n_layers, ou, mid.FMT_RGBA8, 1, t)
        assert rc == 1
        assert b"context is NULL" in mid.lib.mid_last_error()
    assert (out == 7).all() and list(t) == [-1.0, -1.0, -1.0]


def test_cli_help_lists_the_animation_filter():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--animation-filter" in r.stdout
    for name in ("bilateral", "linear", "layers", "nlm"):
        assert name in r.stdout.split("--animation-filter", 1)[1]


def test_cli_refuses_an_unknown_animation_filter(tmp_path):
    r = subprocess.run([CLI, "x.png", "--animation", "--animation-filter", "median"], capture_output=True, text=True,
                       timeout=60, cwd=tmp_path)
    assert r.returncode != 0 and "median" in r.stderr
