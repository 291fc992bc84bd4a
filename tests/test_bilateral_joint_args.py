"""CPU suite: the joint (cross) bilateral (mid_bilateral_joint, mid_sequence_bilateral_joint) is exported and bound as the header
declares it, refuses a NULL context before doing anything, and the CLI offers it as --modes joint, --animation-filter joint /
joint-temporal and --sigma-layers; the float64 checker of the GPU tests (np_bilateral_joint.py) reproduces three answers that need
no kernel: one layer is the layered bilateral, a layer twice at sigma * sqrt 2 is the layer once at sigma, an all-zero layer is
no layer."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import image_denoising_filter_amd as mid
import np_bilateral_joint as chk
import np_bilateral_temporal as layered

CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
ARGC = {"mid_bilateral_joint": 13, "mid_sequence_bilateral_joint": 14}
RTOL = 1e-12                      # the project's bound for its float64 checkers


def _close(a, b):
    return np.abs(a - b).max() <= RTOL * max(1.0, np.abs(b).max())


def _frames(rng, n, h, w):
    return [rng.random((h, w, 4)).astype(np.float32) for _ in range(n)]


def _guides(rng, L, h, w, shift=0):
    yy, xx = np.mgrid[0:h, 0:w]
    return [np.clip(np.stack([xx * 9 + i + shift, yy * 11, (xx + yy) * 5, np.full_like(xx, 255)], -1) + rng.integers(0, 6, (h, w, 4)), 0, 255)
            .astype(np.uint8) for i in range(L)]


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
    for m in ("bilateral_joint", "sequence_bilateral_joint", "sequence_bilateral_joint_pinned"):
        assert hasattr(mid.Context, m)
    assert "MID_VERSION 100" in open(os.path.join(ROOT, "include", "mi_denoise.h")).read()


def test_null_context_is_refused_and_nothing_is_written():
    h, w = 8, 16
    img = np.ones((h, w, 4), np.float32)
    lyr = np.zeros((h, w, 4), np.uint8)
    out = np.full((h, w, 4), 7, np.uint8)
    p = mid.BilateralParams(w, h, 2.0, 0.2, 4, mid.LAYOUT_TEXTURE, mid.FMT_RGBA32F)
    fr = (ctypes.c_void_p * 1)(img.ctypes.data)
    lt = (ctypes.c_void_p * 1)(lyr.ctypes.data)
    ou = (ctypes.c_void_p * 1)(out.ctypes.data)
    sg = (ctypes.c_float * 1)(0.2)
    for sigmas in (sg, None):
        assert mid.lib.mid_bilateral_joint(None, ctypes.byref(p), sigmas, fr, lt, 1, 1, 0, 0, 1, ou, mid.FMT_RGBA8, None) == 1
        assert b"context is NULL" in mid.lib.mid_last_error()
        t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
        assert mid.lib.mid_sequence_bilateral_joint(None, ctypes.byref(p), sigmas, fr, 1, lt, 1, 0, 0, 1, ou, mid.FMT_RGBA8, 1, t) == 1
        assert b"context is NULL" in mid.lib.mid_last_error()
        assert (out == 7).all() and list(t) == [-1.0, -1.0, -1.0] and sg[0] == np.float32(0.2)


def test_cli_offers_the_joint_modes_and_sigma_layers(tmp_path):
    frame = np.full((4, 8, 4), 200, np.uint8)
    for i in range(2):      # (the PNG codec is host code: two tiny frames for the refusal that comes after frame discovery)
        assert mid.lib.mid_image_save(str(tmp_path / f"f_{i:04d}.png").encode(), frame.ctypes.data, 8, 4, mid.FMT_RGBA8) == 0
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    modes = r.stdout.split("--modes", 1)[1].split("--gpu-only", 1)[0]
    assert re.search(r"(?<![-\w])joint(?![-\w])", modes) and "output-nonlinear-bialteral-joint" in modes
    anim = r.stdout.split("--animation-filter", 1)[1].split("--gpus", 1)[0]
    assert re.search(r"(?<![-\w])joint(?![-\w])", anim) and re.search(r"(?<![-\w])joint-temporal", anim)
    assert "output-animation-nonlinear-bialteral-joint-" in anim and "output-animation-nonlinear-bialteral-joint-multiframe-" in anim
    assert re.search(r"^  --sigma-layers ", r.stdout, flags=re.M)
    for value in ("joint", "joint-temporal"):
        # the value is accepted (the run then stops at the missing file, not at the option) ...
        r = subprocess.run([CLI, "/nonexistent/f_0000.png", "--animation", "--animation-filter", value, "--sigma-layers", "0.3,0.5"],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "unknown" not in r.stdout + r.stderr
        # ... needs --animation ...
        r = subprocess.run([CLI, "/nonexistent/f_0000.png", "--animation-filter", value], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--animation" in r.stdout + r.stderr
        # ... and has no RCCL halo exchange
        r = subprocess.run([CLI, str(tmp_path / "f_0000.png"), "--animation", "--animation-filter", value, "--halo", "rccl", "--gpu-only",
                            "--outdir", str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--halo rccl is not available with --animation-filter " + value in r.stdout + r.stderr
        assert not list(tmp_path.glob("output-*"))
    r = subprocess.run([CLI, "/nonexistent/f_0000.png", "--animation", "--animation-filter", "jointx"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "unknown --animation-filter" in r.stdout + r.stderr
    m = re.search(r"unknown --animation-filter[^\n]*", r.stdout + r.stderr).group(0)
    assert "joint-temporal" in m and re.search(r"(?<![-\w])joint(?![-\w])", m.replace("jointx", ""))
    # --modes joint is accepted as well: the run stops at the missing image
    r = subprocess.run([CLI, "/nonexistent/f_0000.png", "--modes", "joint", "--gpu-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "unknown" not in r.stdout + r.stderr and "usage:" not in r.stdout


@pytest.mark.parametrize("k", [0, 1, 2])
def test_checker_with_one_layer_is_the_layered_bilateral(k):
    rng = np.random.default_rng(71)
    h, w, n, R = 13, 19, 4, 3
    frames = _frames(rng, n, h, w)
    layers = [_guides(rng, 1, h, w, 3 * f) for f in range(n)]
    got = chk.bilateral_joint(frames, layers, [0.2], k, R, 2.0)
    want = layered.bilateral_temporal(frames, k, R, 2.0, 0.2, layers=layers, dev=torch.device("cpu"))
    assert len(got) == len(want) == n
    for t in range(n):
        assert _close(got[t], want[t]), t
    sub = chk.bilateral_joint(frames, layers, [0.2], k, R, 2.0, first=1, count=2)
    assert len(sub) == 2 and np.array_equal(sub[0], got[1]) and np.array_equal(sub[1], got[2])


def test_checker_a_layer_twice_at_sigma_sqrt2_is_the_layer_once_at_sigma():
    # exp(-d^2 / (2 (s sqrt 2)^2))^2 = exp(-d^2 / (2 s^2))
    rng = np.random.default_rng(72)
    h, w, n, R = 13, 19, 3, 3
    frames = _frames(rng, n, h, w)
    layers = [_guides(rng, 2, h, w, 3 * f) for f in range(n)]
    s = 0.3
    once = chk.bilateral_joint(frames, layers, [s, 0.4], 1, R, 2.0)
    twice = chk.bilateral_joint(frames, [[ls[0], ls[0], ls[1]] for ls in layers], [s * np.sqrt(2.0), s * np.sqrt(2.0), 0.4], 1, R, 2.0)
    for t in range(n):
        assert _close(twice[t], once[t]), t
    other = chk.bilateral_joint(frames, layers, [s * np.sqrt(2.0), 0.4], 1, R, 2.0)
    assert not _close(other[1], once[1])                   # (the sigma does matter)


def test_checker_an_appended_zero_layer_changes_nothing_exactly():
    rng = np.random.default_rng(73)
    h, w, n, R = 13, 19, 3, 3
    frames = _frames(rng, n, h, w)
    layers = [_guides(rng, 2, h, w, 3 * f) for f in range(n)]
    zero = np.zeros((h, w, 4), np.uint8)
    a = chk.bilateral_joint(frames, layers, [0.2, 0.5], 1, R, 2.0)
    b = chk.bilateral_joint(frames, [ls + [zero] for ls in layers], [0.2, 0.5, 0.01], 1, R, 2.0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_checker_follows_ieee_for_non_finite_guides():
    h, w = 5, 6
    frames = [np.ones((h, w, 4), np.float32)]
    g = np.zeros((h, w, 4), np.float32)
    g[2, 3, 0] = np.inf
    out = chk.bilateral_joint(frames, [[g]], [0.5], 0, 1, 2.0)[0]
    assert np.isnan(out[2, 3]).all() and np.isnan(out).sum() == 4            # Inf - Inf at its own pixel, weight 0 from the others
    assert np.allclose(out[2, 1], [1, 1, 1, 1])                              # (a window inside the image that does not hold it)
    g[2, 3, 0] = np.nan
    out = chk.bilateral_joint(frames, [[g]], [0.5], 0, 1, 2.0)[0]
    assert np.isnan(out[1:4, 2:5]).all() and np.isnan(out).sum() == 36       # a NaN texel poisons every pixel whose window holds it
