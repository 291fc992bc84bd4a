"""CPU suite: the edge-avoiding a-trous filter (mid_atrous_joint, mid_sequence_atrous_joint, mid_atrous_scratch_bytes;
include/mi_denoise.h, section a4g) is exported and bound as the header declares it, mid_atrous_params has the header's layout,
the scratch size is 0 / 1 / 2 float frames, a NULL context is refused before anything is touched, and the class table of the
header, of DESIGN 3.10 and the dispatcher of csrc/atrous.hip agree.  The float64 checker of the GPU tests (np_atrous_joint.py)
keeps a constant frame constant, is the renormalised B3 blur under constant guides, and chains pass by pass."""
import ctypes
import os
import re

import numpy as np

from conftest import ROOT

import image_denoising_filter_amd as mid
import np_atrous_joint as chk

ARGC = {"mid_atrous_joint": 10, "mid_sequence_atrous_joint": 13, "mid_atrous_scratch_bytes": 1}
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
    for m in ("atrous_joint", "sequence_atrous_joint", "sequence_atrous_joint_pinned"):
        assert hasattr(mid.Context, m)


def test_the_ctypes_struct_has_the_layout_of_the_header():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = re.search(r"typedef struct mid_atrous_params \{(.*?)\} mid_atrous_params;", src, flags=re.S).group(1)
    fields = []
    for typ, names in re.findall(r"(int32_t|float)\s+([^;]+);", body):
        fields += [(n.strip(), typ) for n in names.split(",")]
    want = [(n, {ctypes.c_int32: "int32_t", ctypes.c_float: "float"}[t]) for n, t in mid.AtrousParams._fields_]
    assert fields == want == [("width", "int32_t"), ("height", "int32_t"), ("first_pass", "int32_t"), ("n_passes", "int32_t"),
                              ("colorSigma", "float"), ("format", "int32_t")]
    assert ctypes.sizeof(mid.AtrousParams) == 24
    assert [getattr(mid.AtrousParams, n).offset for n, _ in want] == [0, 4, 8, 12, 16, 20]


def test_scratch_is_zero_one_or_two_float_frames():
    w, h = 37, 11
    frame = w * h * 16
    for passes, frames in [(1, 0), (2, 1), (3, 2), (5, 2), (8, 2)]:
        p = mid.AtrousParams(w, h, 0, passes, 0.0, mid.FMT_RGBA8)
        assert mid.lib.mid_atrous_scratch_bytes(ctypes.byref(p)) == frames * frame, passes
    assert mid.lib.mid_atrous_scratch_bytes(None) == 0


def test_null_context_is_refused_and_nothing_is_written():
    h, w = 8, 16
    img = np.ones((h, w, 4), np.float32)
    lyr = np.zeros((h, w, 4), np.uint8)
    out = np.full((h, w, 4), 7, np.uint8)
    p = mid.AtrousParams(w, h, 0, 1, 0.0, mid.FMT_RGBA32F)
    lt = (ctypes.c_void_p * 1)(lyr.ctypes.data)
    sg = (ctypes.c_float * 1)(0.2)
    assert mid.lib.mid_atrous_joint(None, ctypes.byref(p), sg, img.ctypes.data, lt, 1, out.ctypes.data, mid.FMT_RGBA8, None, None) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    fr = (ctypes.c_void_p * 1)(img.ctypes.data)
    ou = (ctypes.c_void_p * 1)(out.ctypes.data)
    t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    assert mid.lib.mid_sequence_atrous_joint(None, ctypes.byref(p), sg, fr, 1, lt, 1, 0, 1, ou, mid.FMT_RGBA8, 1, t) == 1
    assert b"context is NULL" in mid.lib.mid_last_error()
    assert (out == 7).all() and list(t) == [-1.0, -1.0, -1.0] and sg[0] == np.float32(0.2)


ROW = (r"(\d+|1\.\.32|64, 128)\s+(\d+|5\.\.16|1\.\.16)\s+(tiled|comb|global)\s+(64 x \d+)\s+(\d+ x \d+|-)\s+(\d+)\s+(\d|-)\s*$")


def _tiled_bytes(step, L):
    return (64 + 4 * step) * (16 + 4 * step) * (16 + 12 * L)


def _comb_bytes(step, L, rows_per_wave):
    return (64 + 4 * step) * (8 * rows_per_wave + 4) * (16 + 12 * L)


def _class_of(step, L):
    """(kernel, tile, LDS tile, LDS bytes) by the rule of csrc/atrous.hip: the fixed-step kernel at steps 1 and 2 where two of its
    workgroups fit a CU, else the row comb (16 rows while two workgroups fit a CU, else 8) up to step 32 and four layers, else
    global taps."""
    if L <= 4 and step <= 2 and 2 * _tiled_bytes(step, L) <= LDS:
        return "tiled", "64 x 16", f"{64 + 4 * step} x {16 + 4 * step}", _tiled_bytes(step, L)
    if L <= 4 and step <= 32:
        P = 2 if 2 * _comb_bytes(step, L, 2) <= LDS else 1
        return "comb", f"64 x {8 * P}", f"{64 + 4 * step} x {8 * P + 4}", _comb_bytes(step, L, P)
    return "global", "64 x 4", "-", 0


def test_class_table_of_the_header_design_and_dispatcher_agree():
    sec = _header().split("---- a4g:", 1)[1].split("---- a5:", 1)[0]
    rows = re.findall(r"^ \*   " + ROW, sec, flags=re.M)
    assert len(rows) == 26
    design = open(os.path.join(ROOT, "DESIGN.md")).read().split("### 3.10", 1)[1].split("\n## ", 1)[0]
    drows = re.findall(r"^    " + ROW, design, flags=re.M)
    assert drows == rows
    # the table is the rule, row by row, and every tile set fits the LDS of a CU
    seen = set()
    for step, L, kern, tile, lds_tile, lds, per_cu in rows[:24]:
        step, L, lds = int(step), int(L), int(lds)
        assert (kern, tile, lds_tile, lds) == _class_of(step, L), (step, L)
        assert 0 < lds <= LDS and int(per_cu) == min(LDS // lds, 4)
        seen.add((step, L))
    assert seen == {(s_, L) for s_ in (1, 2, 4, 8, 16, 32) for L in (1, 2, 3, 4)}
    assert rows[24] == ("1..32", "5..16", "global", "64 x 4", "-", "0", "-") and rows[25] == ("64, 128", "1..16", "global", "64 x 4", "-", "0", "-")
    assert _class_of(64, 1)[0] == _class_of(128, 4)[0] == _class_of(1, 5)[0] == _class_of(32, 16)[0] == "global"
    # the rule, as the dispatcher's source states it
    src = open(os.path.join(ROOT, "image_denoising_filter_amd", "csrc", "atrous.hip")).read()
    assert "constexpr int kAtrousTiledLayers = 4;" in src and "constexpr int kANW = 8, kAP = 2;" in src and "constexpr int kAtrousCuLds = 163840;" in src
    assert "#define MID_ATROUS_TILED_MAX_STEP 2\n" in src and "#define MID_ATROUS_COMB_MAX_STEP 32\n" in src
    assert ("return step <= kAtrousTiledMaxStep && n_layers <= kAtrousTiledLayers && 2 * atrous_lds_bytes(step, n_layers) <= kAtrousCuLds &&\n"
            "           (int)atrous_lds_bytes(step, n_layers) <= lds_max;") in src
    assert "(size_t)(64 + 4 * step) * (kANW * kAP + 4 * step) * (sizeof(float4) + 3 * sizeof(float) * (size_t)n_layers)" in src
    assert "(size_t)(64 + 4 * step) * (kANW * rows_per_wave + 4) * (sizeof(float4) + 3 * sizeof(float) * (size_t)n_layers)" in src
    assert "constexpr int atrous_comb_rows(int step, int n_layers) { return 2 * atrous_comb_lds_bytes(step, n_layers, 2) <= kAtrousCuLds ? 2 : 1; }" in src
    assert ("return step <= kAtrousCombMaxStep && n_layers <= kAtrousTiledLayers &&\n"
            "           (int)atrous_comb_lds_bytes(step, n_layers, atrous_comb_rows(step, n_layers)) <= lds_max;") in src
    # the dispatcher: tiled, else comb, else global, decided per pass from the step and the layer count alone
    disp = src.split("int dispatch_atrous(", 1)[1].split("\n}\n", 1)[0]
    order = [disp.index(x) for x in ("if (atrous_tiled(ctx->lds_max, a.step, a.n_layers))", "case 1: return launch_atrous_tiled<1>(ctx, a, s);",
                                     "case 2: return launch_atrous_tiled<2>(ctx, a, s);", "if (atrous_comb(ctx->lds_max, a.step, a.n_layers))",
                                     "launch_atrous_comb<2>(ctx, a, s) : launch_atrous_comb<1>(ctx, a, s);",
                                     "atrous_global_kernel, dim3(cdiv(a.w, 64), cdiv(a.h, 4)), dim3(256)")]
    assert order == sorted(order)
    assert "n_passes" not in disp and "first_pass" not in disp


# ---- the float64 checker -------------------------------------------------------------------------------------------------------
def _inputs(rng, h, w, L):
    frame = np.concatenate([rng.random((h, w, 3)) * 4, np.ones((h, w, 1))], -1).astype(np.float32)
    layers = [rng.normal(0, 0.6, (h, w, 4)).astype(np.float32) for _ in range(L)]
    return frame, layers


def test_checker_keeps_a_constant_frame_constant():
    rng = np.random.default_rng(5)
    _, layers = _inputs(rng, 23, 31, 3)
    frame = np.broadcast_to(np.array([0.3, 2.5, 0.01, 0.7], np.float32), (23, 31, 4)).copy()
    for cs in (0.0, 1.0):
        got = chk.atrous_joint(frame, layers, [0.5, 1.0, 0.25], passes=8, color_sigma=cs)
        assert np.abs(got - frame.astype(np.float64)).max() <= 2e-7


def test_checker_one_pass_with_constant_guides_is_the_renormalised_b3_blur():
    rng = np.random.default_rng(6)
    h, w = 13, 17
    frame, _ = _inputs(rng, h, w, 1)
    layers = [np.full((h, w, 4), 0.3, np.float32), np.full((h, w, 4), 7, np.uint8)]
    k1 = np.array([1, 4, 6, 4, 1]) / 16
    for pass_, step in ((0, 1), (2, 4)):
        got = chk.atrous_joint(frame, layers, [0.1, 0.2], passes=1, first_pass=pass_)
        want = np.zeros((h, w, 4))
        for y in range(h):
            for x in range(w):
                num, den = np.zeros(4), 0.0
                for j in range(-2, 3):
                    for i in range(-2, 3):
                        yy, xx = y + j * step, x + i * step
                        if 0 <= yy < h and 0 <= xx < w:
                            num += k1[i + 2] * k1[j + 2] * frame[yy, xx].astype(np.float64)
                            den += k1[i + 2] * k1[j + 2]
                want[y, x] = num / den
        assert np.abs(got - want).max() <= 1e-14


def test_checker_passes_chain():
    rng = np.random.default_rng(7)
    frame, layers = _inputs(rng, 19, 27, 2)
    sig = [0.5, 1.5]
    for cs in (0.0, 2.0):
        for n in (2, 3, 5):
            whole = chk.atrous_joint(frame, layers, sig, passes=n, color_sigma=cs)
            level = frame.astype(np.float64)
            for i in range(n):
                level = chk.atrous_joint(level, layers, sig, passes=1, first_pass=i, color_sigma=cs)
            assert np.array_equal(whole, level), (cs, n)


def test_checker_skips_taps_outside_the_image():
    # a 5 x 7 frame: from step 8 on every tap but the centre is skipped, and the pass is the identity
    rng = np.random.default_rng(8)
    frame, layers = _inputs(rng, 5, 7, 1)
    got = chk.atrous_joint(frame, layers, [0.5], passes=2, first_pass=3)
    assert np.array_equal(got, frame.astype(np.float64))
