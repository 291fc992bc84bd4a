"""CPU suite: the a-trous filter over neighbouring frames (mid_atrous_joint_temporal, mid_sequence_atrous_joint_temporal;
include/mi_denoise.h, section a4h) is exported and bound as the header declares it, a NULL context is refused before anything is
touched, and the float64 checker of the GPU tests (np_atrous_temporal.py) is np_atrous_joint's with a window of one frame and
gives two answers known in closed form."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

import image_denoising_filter_amd as mid
import np_atrous_joint as single
import np_atrous_temporal as chk

ARGC = {"mid_atrous_joint_temporal": 14, "mid_sequence_atrous_joint_temporal": 14}


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
    for m in ("atrous_joint_temporal", "sequence_atrous_joint_temporal", "sequence_atrous_joint_temporal_pinned"):
        assert hasattr(mid.Context, m)


def test_null_context_is_refused_and_nothing_is_written():
    h, w = 8, 16
    img = np.ones((h, w, 4), np.float32)
    lyr = np.zeros((h, w, 4), np.uint8)
    out = np.full((h, w, 4), 7, np.uint8)
    p = mid.AtrousParams(w, h, 0, 1, 0.0, mid.FMT_RGBA32F)
    fr = (ctypes.c_void_p * 1)(img.ctypes.data)
    lt = (ctypes.c_void_p * 1)(lyr.ctypes.data)
    ou = (ctypes.c_void_p * 1)(out.ctypes.data)
    sg = (ctypes.c_float * 1)(0.2)
    assert mid.lib.mid_atrous_joint_temporal(None, ctypes.byref(p), sg, fr, lt, 1, 1, 1, 0, 1, ou, mid.FMT_RGBA8, None, None) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    assert mid.lib.mid_sequence_atrous_joint_temporal(None, ctypes.byref(p), sg, fr, 1, lt, 1, 1, 0, 1, ou, mid.FMT_RGBA8, 1, t) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    assert (out == 7).all() and list(t) == [-1.0, -1.0, -1.0] and sg[0] == np.float32(0.2)


def _inputs(rng, h, w, L, n):
    frames = [np.concatenate([rng.random((h, w, 3)) * 4, np.ones((h, w, 1))], -1).astype(np.float32) for _ in range(n)]
    layers = [[rng.normal(0, 0.6, (h, w, 4)).astype(np.float32) for _ in range(L)] for _ in range(n)]
    return frames, layers


def test_checker_with_a_window_of_one_frame_is_the_single_frame_checker():
    rng = np.random.default_rng(9)
    frames, layers = _inputs(rng, 19, 27, 2, 3)
    sig = [0.5, 1.5]
    for cs in (0.0, 2.0):
        for n in (1, 2, 5):
            got = chk.atrous_joint_temporal(frames, layers, sig, 0, passes=n, color_sigma=cs)
            for t in range(3):
                assert np.array_equal(got[t], single.atrous_joint(frames[t], layers[t], sig, passes=n, color_sigma=cs)), (cs, n, t)
            one = chk.atrous_joint_temporal(frames[1:2], layers[1:2], sig, 2, passes=n, color_sigma=cs)       # n_frames = 1, any k
            assert np.array_equal(one[0], got[1])


def _constant_frames(h, w):
    return [np.full((h, w, 4), c, np.float32) for c in (0.25, 0.5, 0.75)]


def test_known_answer_a_constant_frames_with_identical_guides_average():
    # the valid-tap sum of K is the same in every frame, so every pixel -- corners included -- is the mean of the three constants
    h, w = 7, 9
    frames = _constant_frames(h, w)
    layers = [[np.full((h, w, 4), 0.3, np.float32)] for _ in range(3)]
    got = chk.atrous_joint_temporal(frames, layers, [0.1], 1, passes=1, first=1, count=1)[0]
    assert np.abs(got - 0.5).max() <= 1e-14


def test_known_answer_b_a_far_layer_takes_its_frame_out():
    # frame 0's layer is 255 (1.0 against 0.0 at sigma 0.02: every weight underflows to 0): output 1 is the mean of frames 1 and 2
    h, w = 7, 9
    frames = _constant_frames(h, w)
    layers = [[np.full((h, w, 4), v, np.uint8)] for v in (255, 0, 0)]
    got = chk.atrous_joint_temporal(frames, layers, [0.02], 1, passes=1, first=1, count=1)[0]
    assert np.abs(got - 0.625).max() <= 1e-14
