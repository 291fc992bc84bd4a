"""CPU: the entry points of the variance-guided a-trous filter (include/mi_denoise.h, section a4i) are exported and bound as
declared, the ctypes structs have the header's layout, the scratch size is what the header says, a NULL context is refused with
nothing written, the class tables of the header agree with the rule of csrc/atrous_variance.hip -- and the inputs that
tests/test_gpu_atrous_variance.py asserts on are well-posed: the float64 formula gives the same result, within
2e-6 max(1, |ref|), when every level and variance plane is rounded to fp32 after each pass.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import atrous_variance_inputs as avi
import image_denoising_filter_amd as mid
from conftest import ROOT

ARGC = {"mid_atrous_moments": 11, "mid_atrous_variance": 12, "mid_atrous_variance_scratch_bytes": 1, "mid_sequence_atrous_variance": 14}
LDS = 163840


def _header():
    return open(os.path.join(ROOT, "include", "mi_denoise.h")).read()


def test_entry_points_are_exported_and_bound_as_declared():
    raw = ctypes.CDLL(mid.LIB_PATH)
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, argc in ARGC.items():
        assert hasattr(raw, name)
        assert name in mid.EXPORTED
        fn = getattr(mid.lib, name)
        assert fn.restype is (ctypes.c_size_t if name.endswith("_bytes") else ctypes.c_int)
        assert len(fn.argtypes) == argc, name
        decl = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert decl, f"{name} is not declared in mi_denoise.h"
        params = [a.strip() for a in decl.group(1).split(",")]
        assert len(params) == argc, (name, params)
        for a, t in zip(params, fn.argtypes):           # an int parameter is bound as c_int, a pointer as a pointer type
            assert (("*" not in a) and a.startswith("int ")) == (t is ctypes.c_int), (name, a, t)
    for m in ("atrous_moments", "atrous_variance", "sequence_atrous_variance", "sequence_atrous_variance_pinned"):
        assert hasattr(mid.Context, m)


def _fields(struct):
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", src, flags=re.S).group(1)
    out = []
    for typ, names in re.findall(r"(int32_t|float)\s+([^;]+);", body):
        out += [(n.strip(), typ) for n in names.split(",")]
    return out


def test_the_ctypes_structs_have_the_layout_of_the_header():
    names = {ctypes.c_int32: "int32_t", ctypes.c_float: "float"}
    V, M = mid.AtrousVarianceParams, mid.AtrousMomentsParams
    assert _fields("mid_atrous_variance_params") == [(n, names[t]) for n, t in V._fields_] == \
        [("width", "int32_t"), ("height", "int32_t"), ("first_pass", "int32_t"), ("n_passes", "int32_t"), ("sigmaLum", "float"),
         ("epsilon", "float"), ("format", "int32_t")]
    assert ctypes.sizeof(V) == 28 and [getattr(V, n).offset for n, _ in V._fields_] == [0, 4, 8, 12, 16, 20, 24]
    assert _fields("mid_atrous_moments_params") == [(n, names[t]) for n, t in M._fields_] == \
        [("width", "int32_t"), ("height", "int32_t"), ("format", "int32_t")]
    assert ctypes.sizeof(M) == 12
    assert ctypes.sizeof(mid.AtrousParams) == 24            # mid_atrous_params keeps its layout


def test_scratch_is_zero_one_or_two_sets_of_a_float_frame_and_a_float_plane():
    w, h = 37, 11
    one = w * h * (16 + 4)
    for passes, sets in [(1, 0), (2, 1), (3, 2), (5, 2), (8, 2)]:
        p = mid.AtrousVarianceParams(w, h, 0, passes, 4.0, 1e-3, mid.FMT_RGBA8)
        assert mid.lib.mid_atrous_variance_scratch_bytes(ctypes.byref(p)) == sets * one, passes
    assert mid.lib.mid_atrous_variance_scratch_bytes(None) == 0


def test_null_context_is_refused_and_nothing_is_written():
    h, w = 8, 16
    img = np.ones((h, w, 4), np.float32)
    lyr = np.zeros((h, w, 4), np.uint8)
    var = np.full((h, w), 3.0, np.float32)
    out = np.full((h, w, 4), 7, np.uint8)
    vout = np.full((h, w), 5.0, np.float32)
    lt = (ctypes.c_void_p * 1)(lyr.ctypes.data)
    sg = (ctypes.c_float * 1)(0.2)
    p = mid.AtrousVarianceParams(w, h, 0, 1, 4.0, 1e-3, mid.FMT_RGBA32F)
    assert mid.lib.mid_atrous_variance(None, ctypes.byref(p), sg, img.ctypes.data, var.ctypes.data, lt, 1, out.ctypes.data, mid.FMT_RGBA8,
                                       vout.ctypes.data, None, None) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    fr = (ctypes.c_void_p * 1)(img.ctypes.data)
    m = mid.AtrousMomentsParams(w, h, mid.FMT_RGBA32F)
    assert mid.lib.mid_atrous_moments(None, ctypes.byref(m), sg, fr, lt, 1, 1, 0, 0, vout.ctypes.data, None) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    ou = (ctypes.c_void_p * 1)(out.ctypes.data)
    t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    assert mid.lib.mid_sequence_atrous_variance(None, ctypes.byref(p), sg, fr, 1, lt, 1, 0, 0, 1, ou, mid.FMT_RGBA8, 1, t) == 1
    assert b"context is NULL" in mid.lib.mid_last_error() and list(t) == [-1.0, -1.0, -1.0]
    assert (out == 7).all() and (vout == 5.0).all() and (var == 3.0).all() and sg[0] == np.float32(0.2)


# ---- the class tables ------------------------------------------------------------------------------------------------------------------
ROW_V = r"layers (\d+)\s+step (\d+)\s+kernel comb\s+pixels (64 x \d+)\s+LDS tile (\d+ x \d+)\s+bytes (\d+)\s+workgroups per CU (\d)\s*$"
ROW_M = r"layers (\d+)\s+kernel tiled\s+pixels 64 x 16\s+LDS tile 70 x 22\s+bytes (\d+)\s+workgroups per CU (\d)"


def _comb_bytes(step, L, rows_per_wave):
    return (64 + 4 * step) * (8 * rows_per_wave + 4) * (16 + 4 + 12 * L)


def test_class_tables_of_the_header_and_the_dispatcher_agree():
    sec = _header().split("---- a4i:", 1)[1].split("---- a5:", 1)[0]
    rows = re.findall(r"^ \*   " + ROW_V, sec, flags=re.M)
    seen = set()
    for L, step, tile, lds_tile, lds, per_cu in rows:
        L, step, lds = int(L), int(step), int(lds)
        P = 2 if 2 * _comb_bytes(step, L, 2) <= LDS else 1
        assert (tile, lds_tile, lds) == (f"64 x {8 * P}", f"{64 + 4 * step} x {8 * P + 4}", _comb_bytes(step, L, P)), (step, L)
        assert 0 < lds <= LDS and int(per_cu) == min(LDS // lds, 4)
        seen.add((step, L))
    assert seen == {(s_, L) for s_ in (1, 2, 4, 8, 16, 32) for L in (1, 2, 3, 4)} and len(rows) == 24
    assert " *   layers 5..16  step 1..32     kernel global  pixels 64 x 4  no LDS\n" in sec
    assert " *   layers 1..16  step 64, 128   kernel global  pixels 64 x 4  no LDS\n" in sec
    mrows = re.findall(r"^ \*   " + ROW_M, sec, flags=re.M)
    assert [(int(L), int(b)) for L, b, _ in mrows] == [(L, 70 * 22 * 4 * (1 + 3 * L)) for L in (1, 2, 3, 4)]
    assert all(int(n) == min(LDS // int(b), 6) for _, b, n in mrows)
    assert " *   layers 5..16   kernel global  pixels 64 x 4   no LDS\n" in sec
    # the rule, as the dispatcher's source states it
    src = open(os.path.join(ROOT, "image_denoising_filter_amd", "csrc", "atrous_variance.hip")).read()
    assert "constexpr int kAVTiledLayers = 4;" in src and "constexpr int kAVNW = 8;" in src and "constexpr int kAVCuLds = 163840;" in src
    assert "constexpr int kAVCombMaxStep = 32;" in src and "constexpr int kMomR = 3;" in src and "constexpr int kMomP = 2;" in src
    assert ("(size_t)(64 + 4 * step) * (kAVNW * rows_per_wave + 4) * (sizeof(float4) + sizeof(float) + 3 * sizeof(float) * (size_t)n_layers)") in src
    assert "constexpr int variance_comb_rows(int step, int n_layers) { return 2 * variance_comb_lds_bytes(step, n_layers, 2) <= kAVCuLds ? 2 : 1; }" in src
    assert ("return step <= kAVCombMaxStep && n_layers <= kAVTiledLayers &&\n"
            "           (int)variance_comb_lds_bytes(step, n_layers, variance_comb_rows(step, n_layers)) <= lds_max;") in src
    assert "constexpr int kMomLW = 64 + 2 * kMomR, kMomLH = kAVNW * kMomP + 2 * kMomR;" in src
    assert "return (size_t)kMomLW * kMomLH * sizeof(float) * (1 + 3 * (size_t)n_layers);" in src
    assert "return n_layers <= kAVTiledLayers && (int)moments_lds_bytes(n_layers) <= lds_max;" in src
    disp = src.split("int dispatch_variance(", 1)[1].split("\n}\n", 1)[0]
    order = [disp.index(x) for x in ("if (variance_comb(ctx->lds_max, a.step, a.n_layers))", "launch_variance_comb<2>(ctx, a, s)",
                                     "launch_variance_comb<1>(ctx, a, s)", "hipLaunchKernelGGL(variance_global_kernel")]
    assert order == sorted(order) and "n_passes" not in disp and "first_pass" not in disp
    disp = src.split("int dispatch_moments(", 1)[1].split("\n}\n", 1)[0]
    assert disp.index("if (moments_tiled(ctx->lds_max, a.n_layers))") < disp.index("hipLaunchKernelGGL(moments_global_kernel")
    # existing kernel sources keep their text: the new kernels restate what they share
    assert "atrous_variance" not in open(os.path.join(ROOT, "image_denoising_filter_amd", "csrc", "atrous.hip")).read()


# ---- conditioning of the GPU test inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", avi.CASES, ids=avi.case_id)
def test_the_inputs_of_the_gpu_test_are_well_posed(case):
    (C, V), (C32, V32) = avi.case_reference(case)
    ec = float(np.max(np.abs(C - C32) / np.maximum(1.0, np.abs(C))))
    ev = float(np.max(np.abs(V - V32) / np.maximum(1.0, np.abs(V))))
    print(f"{avi.case_id(case)}: colour {ec:.2e}, variance {ev:.2e}")
    assert np.isfinite(C).all() and np.isfinite(V).all() and V.min() >= 0
    assert ec <= 2e-6 and ev <= 2e-6, (ec, ev)
