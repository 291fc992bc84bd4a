"""CPU suite: every layer carries the guided filter (section a4o) -- header, library, EXPORTED table, Context, the CLI's --help --, the
keywords are refused before any GPU work, the workspace query against its stated bound, the CLI's refusals that need no device, and
the recipe of the GPU tests (tests/guided_inputs.py) meets its conditions by the float64 checker alone."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import image_denoising_filter_amd as mid
import guided_inputs as gi
import np_guided

NEW = ("mid_guided_workspace", "mid_guided_filter", "mid_sequence_guided")
CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")


def test_header_library_and_table_carry_the_new_entry_points():
    src = open(os.path.join(ROOT, "include", "mi_denoise.h")).read()
    assert "a4o" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(mid.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), f"{name} is not declared in mi_denoise.h"
        assert hasattr(raw, name), f"{name} is not exported by libmi_denoise.so"
        assert name in mid.EXPORTED
    assert re.search(r"typedef struct mid_guided_params \{\s*int32_t width, height;\s*int32_t radius;\s*float\s+eps;\s*int32_t format;\s*\} mid_guided_params;", code)
    P = mid.GuidedParams
    assert (P.width.offset, P.height.offset, P.radius.offset, P.eps.offset, P.format.offset, ctypes.sizeof(P)) == (0, 4, 8, 12, 16, 20)
    assert "GuidedParams" in mid.__all__
    # the geometry the tests are written for is the geometry built
    box = open(os.path.join(ROOT, "image_denoising_filter_amd", "csrc", "guided_box.hpp")).read()
    assert f"kGuidedLanes = {gi.LANES};" in box and f"kGuidedPeriod = {gi.PERIOD};" in box and "kGuidedMaxRadius = 16;" in box


def test_the_python_layer_has_the_keywords_and_their_defaults():
    sig = inspect.signature(mid.Context.guided_filter).parameters
    assert list(sig) == ["self", "frame", "guide", "radius", "eps", "out_dtype"]
    assert [sig[k].default for k in ("guide", "radius", "eps", "out_dtype")] == [None, 8, 1e-2, None]
    sig = inspect.signature(mid.Context.sequence_guided).parameters
    assert list(sig) == ["self", "frames", "guides", "radius", "eps", "first", "count", "overlap", "pinned", "out_dtype"]
    assert [sig[k].default for k in list(sig)[2:]] == [None, 8, 1e-2, 0, None, True, True, None]
    assert hasattr(mid.Context, "sequence_guided_pinned")


def test_bad_arguments_raise_before_any_gpu_work():
    """The methods are called without a context (self = None): a ValueError must come before anything touches it."""
    f = np.zeros((4, 5, 4), np.float32)
    for call in (lambda **kw: mid.Context.guided_filter(None, f, f, **kw), lambda **kw: mid.Context.sequence_guided(None, [f, f], [f, f], **kw)):
        for r in (0, -1, 17, 2.0, None, True, "3"):
            with pytest.raises(ValueError, match="radius must be an integer in 1..16"):
                call(radius=r)
        for e in (0, -1e-2, float("nan"), float("inf"), None, True, "1", 1e39, 1e-50):
            with pytest.raises(ValueError, match="eps must be"):
                call(eps=e)
        for dt in (np.float64, np.int32, "bfloat"):
            with pytest.raises((ValueError, TypeError), match="out_dtype|data type"):
                call(out_dtype=dt)
    with pytest.raises(ValueError, match="one size"):
        mid.Context.guided_filter(None, f, np.zeros((5, 4, 4), np.float32))
    with pytest.raises(ValueError, match=r"\(h, w, 4\)"):
        mid.Context.guided_filter(None, f[..., :3])
    for bad in (np.float64, np.int32, np.uint16):
        with pytest.raises(ValueError, match="uint8 / float16 / float32"):
            mid.Context.guided_filter(None, f, f.astype(bad))
        with pytest.raises(ValueError, match="uint8 / float16 / float32"):
            mid.Context.guided_filter(None, f.astype(bad))
        with pytest.raises(ValueError, match="uint8 / float16 / float32"):
            mid.Context.sequence_guided(None, [f.astype(bad)])
        with pytest.raises(ValueError, match="uint8 / float16 / float32"):
            mid.Context.sequence_guided(None, [f], [f.astype(bad)])
    with pytest.raises(ValueError, match="1 guides for 2 frames"):
        mid.Context.sequence_guided(None, [f, f], [f])
    with pytest.raises(ValueError):
        mid.Context.sequence_guided(None, [f, f], [f, np.zeros((5, 4, 4), np.float32)])
    with pytest.raises(ValueError):
        mid.Context.sequence_guided(None, [f, np.zeros((5, 4, 4), np.float32)])


def test_workspace_query_needs_no_device_and_keeps_its_bound():
    n = ctypes.c_size_t()
    for w, h in ((1, 1), (5, 3), (1920, 1080), (16400, 16400), (262149, 1), (1, 70000)):
        for r in (1, 16):
            p = mid.GuidedParams(w, h, r, 1e-2, mid.FMT_RGBA8)
            assert mid.lib.mid_guided_workspace(ctypes.byref(p), ctypes.byref(n)) == 0
            assert n.value == 52 * w * h <= 64 * w * h              # the header: 52 bytes per pixel, no constant; the contract allows 64
    for kw in (dict(width=0), dict(height=-1), dict(width=1 << 15, height=1 << 15), dict(radius=0), dict(radius=17), dict(eps=0.0),
               dict(eps=float("nan")), dict(format=3), dict(format=1 << 16)):
        p = mid.GuidedParams(**{**dict(width=8, height=8, radius=2, eps=1e-2, format=mid.FMT_RGBA32F), **kw})
        n.value = 777
        assert mid.lib.mid_guided_workspace(ctypes.byref(p), ctypes.byref(n)) == 1 and n.value == 777, kw


def test_help_lists_the_options():
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("\n  --guided-radius R ", "\n  --guided-eps X ", "\n  --guide-layer SUBSTR ", "output-nonlinear-guided.{png,exr}",
                "output-animation-nonlinear-guided-*"):
        assert opt in h, opt


def test_the_cli_refuses_what_it_cannot_mean():
    """Refusals that come before any file or device is touched."""
    for extra, word in ((["--guided-radius", "3"], "--guided-radius applies to --modes guided"), (["--guided-eps", "0.1"], "--guided-eps applies to"),
                        (["--guide-layer", "albedo"], "--guide-layer applies to"),
                        (["--modes", "atrous", "--guide-layer", "albedo"], "--guide-layer applies to"),
                        (["--animation", "--animation-filter", "atrous", "--guided-radius", "3"], "--guided-radius applies to"),
                        (["--animation", "--modes", "guided", "--guided-radius", "3"], "--guided-radius applies to")):
        r = subprocess.run([CLI, "--cpu-only"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr)
    for extra, word in ((["--guided-radius", "0"], "is outside 1..16"), (["--guided-radius", "17"], "is outside 1..16"), (["--guided-eps", "0"], "must be finite and > 0"),
                        (["--guided-eps", "nan"], "must be finite and > 0"), (["--guided-eps", "inf"], "must be finite and > 0"), (["--guided-eps", "-1"], "must be finite and > 0")):
        r = subprocess.run([CLI, "--modes", "guided"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr)
    r = subprocess.run([CLI, "--animation", "--animation-filter", "guide"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "unknown --animation-filter guide" in r.stderr and "guided" in r.stderr


@pytest.mark.parametrize("radius", gi.RADII)
def test_the_recipe_meets_its_conditions(radius):
    """At the shapes the GPU tests spend most of their pixels on, for float and u8 guides."""
    for h, w in ((70, 261), (131, 250)):
        noisy, alb, clean = gi.scene(h, w, radius, seed=h * 1000 + w)
        assert noisy.dtype == np.float32 and np.isfinite(noisy).all() and np.isfinite(alb).all()
        for guide in (alb, gi.as_dtype(alb, np.uint8)):
            ref = np_guided.guided(noisy, guide, radius, gi.EPS)
            lam = ref["lam_max"]
            flat, active = float((lam <= gi.EPS / 10).mean()), float((lam >= 10 * gi.EPS).mean())
            changed = float((np.abs(ref["out"][..., :3] - noisy[..., :3].astype(np.float64)).max(-1) > 0.05).mean())
            t_rel = float((ref["T"] / np.maximum(1.0, np.abs(ref["out"][..., :3]))).max())
            print(f"r={radius} {w}x{h} {guide.dtype}: flat {flat:.2f} active {active:.2f} changed {changed:.2f} T/|out| {t_rel:.1f}")
            if min(h, w) >= 8 * radius:                             # (a frame of less than two blocks has no flat window to speak of)
                assert flat >= 0.1
            assert active >= 0.1 and changed > 0.5 and t_rel <= 64
            # the precision clause: D^2 / eps <= 2^10 n_min, D the largest deviation of a guide channel from ANY texel of the frame
            G = np_guided.widen(guide)[..., :3]
            D = float((G.max((0, 1)) - G.min((0, 1))).max())
            assert D * D / gi.EPS <= 2 ** 10 * float(ref["n"].min()) and ref["n"].min() == (radius + 1) ** 2
    d = gi.depth_guide(70, 257, radius)
    G = d[..., :3].astype(np.float64)
    D = float((G.max((0, 1)) - G.min((0, 1))).max())
    assert 200 < G.min() and D <= 30 and D * D / gi.DEPTH_EPS <= 2 ** 10 * (radius + 1) ** 2
    ref = np_guided.guided(gi.scene(70, 257, radius, seed=70257)[0], d, radius, gi.DEPTH_EPS)
    assert float((ref["T"] / np.maximum(1.0, np.abs(ref["out"][..., :3]))).max()) <= 64 * 300     # b carries the guide's offset: T is in ITS units
    assert float((ref["lam_max"] >= 10 * gi.DEPTH_EPS).mean()) >= 0.1


def test_the_demonstration_in_float64():
    """What tests/test_gpu_guided_demo.py asserts of the kernel is true of the contract: guided by the clean albedo the output is much
    closer to the clean frame than the input; guided by itself it is not."""
    noisy, alb, clean = gi.demo()
    c = clean[..., :3].astype(np.float64)
    mse = lambda x: float(((x[..., :3] - c) ** 2).mean())
    m_in = mse(noisy.astype(np.float64))
    m_guided = mse(np_guided.guided(noisy, alb, gi.DEMO_RADIUS, gi.DEMO_EPS)["out"])
    m_self = mse(np_guided.guided(noisy, None, gi.DEMO_RADIUS, gi.DEMO_EPS)["out"])
    print(f"mse: input {m_in:.5f}, guided {m_guided:.5f}, self-guided {m_self:.5f}")
    assert m_guided <= gi.DEMO_GUIDED_RATIO * m_in * (1 - 1e-3)
    assert m_self >= gi.DEMO_SELF_RATIO * m_guided * (1 + 1e-3)
