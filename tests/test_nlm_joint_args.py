"""CPU suite: joint layer-guided NLM (mid_nlm_joint, mid_sequence_nlm_joint; include/mi_denoise.h, section a4f) is exported and
bound as the header declares it, refuses a NULL context before doing anything, and the CLI offers it as --modes nlm-joint,
--animation-filter nlm-joint / nlm-joint-temporal and --h-layers.  The float64 checker of the GPU tests (np_nlm_joint.py) equals the
layered checker with one layer, reproduces a known answer derived by hand, and differs from the layered checker where a joint weight
must; the class table of the header is held against the constants of csrc/nlm_joint.hip and against the LDS arithmetic."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import image_denoising_filter_amd as mid
import np_nlm_joint as chk
import np_nlm_layers_temporal as layered

CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
ARGC = {"mid_nlm_joint": 13, "mid_sequence_nlm_joint": 14}
RTOL = 1e-12                      # the project's bound for its float64 checkers
LDS = 163840


def _close(a, b):
    return np.abs(a - b).max() <= RTOL * max(1.0, np.abs(b).max())


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
    for m in ("nlm_joint", "sequence_nlm_joint", "sequence_nlm_joint_pinned"):
        assert hasattr(mid.Context, m)


def test_null_context_is_refused_and_nothing_is_written():
    h, w = 8, 16
    img = np.ones((h, w, 4), np.float32)
    lyr = np.zeros((h, w, 4), np.uint8)
    out = np.full((h, w, 4), 7, np.uint8)
    p = mid.NlmParams(w, h, 0.5, -7, 7, -3, 3, mid.FMT_RGBA32F)
    fr = (ctypes.c_void_p * 1)(img.ctypes.data)
    lt = (ctypes.c_void_p * 1)(lyr.ctypes.data)
    ou = (ctypes.c_void_p * 1)(out.ctypes.data)
    hh = (ctypes.c_float * 1)(0.2)
    for hs in (hh, None):
        assert mid.lib.mid_nlm_joint(None, ctypes.byref(p), hs, fr, lt, 1, 1, 0, 0, 1, ou, mid.FMT_RGBA8, None) == 1
        assert b"context is NULL" in mid.lib.mid_last_error()
        t = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
        assert mid.lib.mid_sequence_nlm_joint(None, ctypes.byref(p), hs, fr, 1, lt, 1, 0, 0, 1, ou, mid.FMT_RGBA8, 1, t) == 1
        assert b"context is NULL" in mid.lib.mid_last_error()
        assert (out == 7).all() and list(t) == [-1.0, -1.0, -1.0] and hh[0] == np.float32(0.2)


def test_cli_offers_the_nlm_joint_modes_and_h_layers(tmp_path):
    frame = np.full((4, 8, 4), 200, np.uint8)
    for i in range(2):      # (the PNG codec is host code: two tiny frames for the refusal that comes after frame discovery)
        assert mid.lib.mid_image_save(str(tmp_path / f"f_{i:04d}.png").encode(), frame.ctypes.data, 8, 4, mid.FMT_RGBA8) == 0
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    modes = r.stdout.split("--modes", 1)[1].split("--gpu-only", 1)[0]
    assert re.search(r"(?<![-\w])nlm-joint(?![-\w])", modes) and "output-nonlinear-nlm-joint.{png,exr}" in modes
    anim = r.stdout.split("--animation-filter", 1)[1].split("--gpus", 1)[0]
    assert re.search(r"(?<![-\w])nlm-joint(?![-\w])", anim) and re.search(r"(?<![-\w])nlm-joint-temporal", anim)
    assert "output-animation-nonlinear-nlm-joint-*" in anim and "output-animation-nonlinear-nlm-joint-multiframe-*" in anim
    assert re.search(r"^  --h-layers ", r.stdout, flags=re.M)
    # the options keep their order
    order = [m.group(1) for m in re.finditer(r"^  (--[\w-]+)", r.stdout, flags=re.M)]
    assert order[order.index("--nlm-h") + 1] == "--h-layers" and order.index("--modes") < order.index("--gpu-only") < order.index("--animation-filter") < order.index("--gpus")
    for value in ("nlm-joint", "nlm-joint-temporal"):
        # the value is accepted (the run then stops at the missing file, not at the option) ...
        r = subprocess.run([CLI, "/nonexistent/f_0000.png", "--animation", "--animation-filter", value, "--h-layers", "0.3,0.5"],
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
    r = subprocess.run([CLI, "/nonexistent/f_0000.png", "--animation", "--animation-filter", "nlm-jointx"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "unknown --animation-filter" in r.stdout + r.stderr
    m = re.search(r"unknown --animation-filter[^\n]*", r.stdout + r.stderr).group(0)
    assert "nlm-joint-temporal" in m and re.search(r"(?<![-\w])nlm-joint(?![-\w])", m.replace("nlm-jointx", ""))
    # --modes nlm-joint is accepted as well: the run stops at the missing image; an empty --h-layers is refused
    r = subprocess.run([CLI, "/nonexistent/f_0000.png", "--modes", "nlm-joint", "--gpu-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "unknown" not in r.stdout + r.stderr and "usage:" not in r.stdout
    r = subprocess.run([CLI, "/nonexistent/f_0000.png", "--modes", "nlm-joint", "--h-layers", ""], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--h-layers needs" in r.stderr


def test_checker_with_one_layer_is_the_layered_checker():
    rng = np.random.default_rng(81)
    h, w, n = 13, 19, 4
    frames = [rng.random((h, w, 4)).astype(np.float32) for _ in range(n)]
    layers = [_guides(rng, 1, h, w, 3 * f) for f in range(n)]
    for k in (0, 1, 2):
        got = chk.nlm_joint(frames, layers, [0.3], k, (-3, 4), (-1, 2))
        want = layered.nlm_layers_temporal(frames, layers, k, 0.3, (-3, 4), (-1, 2))
        assert len(got) == len(want) == n
        for t in range(n):
            assert _close(got[t], want[t]), (k, t)
    sub = chk.nlm_joint(frames, layers, [0.3], 1, (-3, 4), (-1, 2), first=1, count=2)
    full = chk.nlm_joint(frames, layers, [0.3], 1, (-3, 4), (-1, 2))
    assert len(sub) == 2 and np.array_equal(sub[0], full[1]) and np.array_equal(sub[1], full[2])


def test_checker_an_appended_zero_layer_changes_nothing_exactly():
    rng = np.random.default_rng(83)
    h, w, n = 13, 19, 2
    frames = [rng.random((h, w, 4)).astype(np.float32) for _ in range(n)]
    layers = [_guides(rng, 2, h, w, 3 * f) for f in range(n)]
    zero = np.zeros((h, w, 4), np.uint8)
    a = chk.nlm_joint(frames, layers, [0.3, 0.7], 1, (-3, 4), (-1, 2))
    b = chk.nlm_joint(frames, [ls + [zero] for ls in layers], [0.3, 0.7, 0.01], 1, (-3, 4), (-1, 2))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_checker_reproduces_the_known_answer_with_a_one_texel_patch():
    frame, guides = chk.known_answer_inputs()
    want, ok, n = chk.known_answer((0, 1))
    assert ok.all() and n.min() == 121 and n.max() == 441
    got = chk.nlm_joint([frame], [guides], chk.KA_HS, 0, (-10, 11), (0, 1))[0]
    assert np.abs(got - want).max() < 1e-14


def test_checker_reproduces_the_known_answer_with_the_tuned_window():
    frame, guides = chk.known_answer_inputs()
    want, ok, n = chk.known_answer((-3, 4))
    assert ok.sum() == 2632
    got = chk.nlm_joint([frame], [guides], chk.KA_HS, 0, (-10, 11), (-3, 4))[0]
    assert np.abs(got - want)[ok].max() < 1e-14


def test_the_layered_sum_is_no_joint_weight():
    # one filter per layer, added, keeps every window pixel that matches in EITHER layer: far from the joint result
    rng = np.random.default_rng(82)
    _, guides = chk.known_answer_inputs()
    frame = rng.random((chk.KA_H, chk.KA_W, 4)).astype(np.float32)
    frame[..., 3] = 1
    lay = layered.nlm_layers_temporal([frame], [guides], 0, 0.02, (-10, 11), (0, 1))[0]
    jo = chk.nlm_joint([frame], [guides], chk.KA_HS, 0, (-10, 11), (0, 1))[0]
    assert np.abs(lay - jo).max() > 1e-3


def _lds_bytes(sw, pw, tile_h, n_layers):
    lw = 64 + sw - 1
    return lw * (tile_h + sw - 1) * 16 + n_layers * lw * (tile_h + pw - 1 + sw - 1) * 4


def test_class_table_of_the_header_matches_the_kernel_source_and_the_lds_arithmetic():
    hdr = open(os.path.join(ROOT, "include", "mi_denoise.h")).read()
    sec = hdr.split("---- a4f:", 1)[1].split("---- a5:", 1)[0]
    rows = re.findall(r"^ \*   (\d+x\d+ / \d+x\d+)\s+(\d)\s+(\d)\s+(\d+)\s+(float|packed)\s+(\d)\s+(\d+)$", sec, flags=re.M)
    assert len(rows) == 8
    src = open(os.path.join(ROOT, "image_denoising_filter_amd", "csrc", "nlm_joint.hip")).read()
    assert re.search(r"constexpr int kJointTiledLayers = 4;", src) and re.search(r"constexpr int kJNW = 8;", src)
    assert re.search(r"constexpr int joint_rows\(int n_layers\) \{ return n_layers == 1 \? 8 : 4; \}", src)
    assert re.search(r"constexpr bool joint_packed\(int n_layers\) \{ return n_layers >= 3; \}", src)
    assert re.search(r"constexpr int joint_packed_targets\(int n_layers\) \{ return n_layers >= 4 \? 1 : 0; \}", src)
    assert "launch_joint_window<-10, 11, -3, 4>" in src and "launch_joint_window<-7, 7, -3, 3>" in src
    assert "default: return launch_joint_generic(p, a, s);" in src
    windows = {"21x21 / 7x7": (21, 7), "14x14 / 6x6": (14, 6)}
    seen = set()
    for win, L, rows_per_wave, tile_h, ring, tp, lds in rows:
        L, rows_per_wave, tile_h, tp, lds = int(L), int(rows_per_wave), int(tile_h), int(tp), int(lds)
        sw, pw = windows[win]
        assert rows_per_wave == (8 if L == 1 else 4) and tile_h == 8 * rows_per_wave
        assert ring == ("packed" if L >= 3 else "float") and tp == (1 if L >= 4 else 0)
        assert lds == _lds_bytes(sw, pw, tile_h, L) <= LDS, (win, L)
        seen.add((win, L))
    assert seen == {(wn, L) for wn in windows for L in (1, 2, 3, 4)}
    # the budgets the shapes were chosen from: with 64-row tiles only one layer fits beside the 21x21 / 7x7 colour tile, two beside
    # the 14x14 / 6x6 one; with 32-row tiles four fit either
    assert _lds_bytes(21, 7, 64, 1) == 112896 + 30240 and _lds_bytes(21, 7, 64, 2) > LDS
    assert _lds_bytes(21, 7, 32, 4) == 69888 + 4 * 19488 == 147840
    assert _lds_bytes(14, 6, 64, 2) == 94864 + 2 * 25256 == 145376 and _lds_bytes(14, 6, 64, 3) > LDS
    # the one-layer class keeps the layered kernel's shape
    lt = open(os.path.join(ROOT, "image_denoising_filter_amd", "csrc", "nlm_layers_temporal.hip")).read()
    assert re.search(r"constexpr int kLR = 8, kLNW = 8;", lt)
