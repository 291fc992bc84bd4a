"""CPU suite: the median filters' arguments and the recipe of their GPU tests (tests/median_inputs.py), held to its conditions by the
float64 checker (tests/np_median.py) alone; the ValueErrors of the Python layer, which come before any GPU work; "every layer carries
the entry points"; the CLI refusals that need no device; and the demonstration's three ratios in float64."""
import os
import subprocess

import numpy as np
import pytest

import image_denoising_filter_amd as mid
import median_inputs as mi
import np_bilateral_joint
import np_median
from conftest import ROOT

CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")


def test_every_layer_carries_the_entry_points():
    for name in ("mid_median_filter", "mid_sequence_median"):
        assert name in mid.EXPORTED and hasattr(mid.lib, name)
        assert name + "(" in open(os.path.join(ROOT, "include", "mi_denoise.h")).read()
    assert [f for f, _ in mid.MedianParams._fields_] == ["width", "height", "radius", "format"]
    for method in ("median_filter", "sequence_median", "sequence_median_pinned"):
        assert callable(getattr(mid.Context, method))
    assert "MedianParams" in mid.__all__
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    for opt in ("\n  --median-radius R ", "\n  --median-plain ", "output-nonlinear-median.{png,exr}", "output-animation-nonlinear-median-*"):
        assert opt in h, opt


def test_value_errors_come_before_any_gpu_work():
    f = np.zeros((4, 5, 4), np.float32)
    g8, g16 = np.zeros((4, 5, 4), np.uint8), np.zeros((4, 5, 4), np.float16)
    for call in (lambda **kw: mid.Context.median_filter(None, f, **kw), lambda **kw: mid.Context.sequence_median(None, [f], **kw)):
        for r in (0, 4, -1, 1.5, "2", True, None):
            with pytest.raises(ValueError, match="radius"):
                call(radius=r)
        with pytest.raises(ValueError, match="sigmas without layers"):
            call(sigmas=[0.1])
        for dt in (np.float64, np.int32):
            with pytest.raises(ValueError, match="out_dtype"):
                call(out_dtype=dt)
    with pytest.raises(ValueError, match="layers without sigmas"):
        mid.Context.median_filter(None, f, [g8])
    with pytest.raises(ValueError, match="2 sigmas for 1 layers"):
        mid.Context.median_filter(None, f, [g8], [0.1, 0.2])
    with pytest.raises(ValueError, match="share one dtype"):
        mid.Context.median_filter(None, f, [g8, g16], [0.1, 0.2])
    with pytest.raises(ValueError, match="share one dtype"):
        mid.Context.sequence_median(None, [f, f], [[g8], [g16]], [0.1])
    with pytest.raises(ValueError, match=r"uint8 / float16 / float32 \(4, 5, 4\)"):
        mid.Context.median_filter(None, f, [np.zeros((5, 4, 4), np.uint8)], [0.1])
    with pytest.raises(ValueError, match=r"uint8 / float16 / float32"):
        mid.Context.median_filter(None, f, [f.astype(np.float64)], [0.1])
    with pytest.raises(ValueError, match=r"\(h, w, 4\)"):
        mid.Context.median_filter(None, f[..., :3])
    with pytest.raises(TypeError, match="float32, uint8 or float16"):
        mid.Context.median_filter(None, f.astype(np.float64))
    with pytest.raises(ValueError, match="1 layer lists for 2 frames"):
        mid.Context.sequence_median(None, [f, f], [[g8]], [0.1])
    with pytest.raises(ValueError, match="frame 1 has 2 layers, frame 0 has 1"):
        mid.Context.sequence_median(None, [f, f], [[g8], [g8, g8]], [0.1])
    with pytest.raises(ValueError, match="frame 1 is"):
        mid.Context.sequence_median(None, [f, np.zeros((5, 4, 4), np.float32)])


def test_the_cli_refuses_what_it_cannot_mean():
    """Refusals that come before any file or device is touched."""
    for extra, word in ((["--median-radius", "2"], "--median-radius applies to --modes median"), (["--median-plain"], "--median-plain applies to"),
                        (["--modes", "atrous", "--median-plain"], "--median-plain applies to"),
                        (["--animation", "--animation-filter", "atrous", "--median-radius", "2"], "--median-radius applies to"),
                        (["--animation", "--modes", "median", "--median-radius", "2"], "--median-radius applies to")):
        r = subprocess.run([CLI, "--cpu-only"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and word in r.stderr, (extra, r.stderr)
    for v in ("0", "4", "-1"):
        r = subprocess.run([CLI, "--modes", "median", "--median-radius", v], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "is outside 1..3" in r.stderr, (v, r.stderr)
    r = subprocess.run([CLI, "--animation", "--animation-filter", "medians"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "unknown --animation-filter medians" in r.stderr and "median" in r.stderr


def gpu_cases():
    """(h, w, radius, n_layers, gain) of every case tests/test_gpu_median.py runs with uint8 guides (the frame's dtype moves no weight;
    the float16 and float32 guides and the other GPU tests' cases: test_the_other_gpu_cases_meet_the_conditions)."""
    cases = set()
    for radius in mi.RADII:
        for n_layers in mi.LAYER_COUNTS:
            cases.update((h, w, radius, n_layers, 1.0) for h, w in mi.seam_shapes(n_layers))
        for n_layers in (0, 3, 5):
            cases.update((h, 37, radius, n_layers, 1.0) for h in range(1, 35))
    for radius, n_layers in ((1, 0), (2, 1), (3, 4), (2, 5)):
        cases.add((35, 131, radius, n_layers, 1.0))
    for radius, n_layers in ((1, 0), (2, 3), (3, 5)):
        cases.add((34, 67, radius, n_layers, 1.0))
    for gain in (1 / 64, 1 / 4, 16.0, 1024.0):
        cases.update((33, 70, radius, n_layers, gain) for radius, n_layers in ((1, 0), (2, 1), (3, 3), (2, 16)))
    return sorted(cases)


def test_the_recipe_meets_its_conditions():
    worst_near, worst_cond = (-1.0, ()), (-1.0, ())
    changed, straddle, pixels, windows = 0.0, 0.0, 0, 0
    for h, w, radius, n_layers, gain in gpu_cases():
        noisy, g0, _ = mi.scene(h, w, seed=h * 1000 + w, gain=gain)
        assert noisy.dtype == np.float32 and np.isfinite(noisy).all()
        layers, sigmas = mi.layer_set(g0, n_layers)
        out, margin, exact = np_median.median(noisy, layers, sigmas, radius)
        near = float(((margin <= np_median.DELTA) & ~exact).mean())
        assert near <= mi.NEAR_SHARE, (h, w, radius, n_layers, near)
        worst_near = max(worst_near, (near, (h, w, radius, n_layers)))
        changed += float((out[..., :3] != noisy[..., :3]).any(-1).sum())
        pixels += h * w
        if n_layers == 0:
            assert exact.all()
            continue
        arg = np_median.tap_args(layers, sigmas, radius, (h, w))
        wt = np_median.tap_weights(layers, sigmas, radius, (h, w))
        W = wt.sum(-1)
        # the header's condition: (3 L' + 2) A <= 295, A the largest |arg| among the taps with w > 2^-24 W (every layer counted live)
        A = float(np.abs(arg[wt > 2.0 ** -24 * W[..., None]]).max())
        cond = (3 * n_layers + 2) * A
        assert cond <= 295, (h, w, radius, n_layers, A)
        worst_cond = max(worst_cond, (cond, (h, w, radius, n_layers)))
        assert not (np.abs(arg + 126.0) < 0.01).any()               # no exponent at the cut arg = -126: fp32 and float64 agree on its side
        if h >= 16 and w >= 16:
            straddle += float((W < (2 * radius + 1) ** 2 / 2).sum())
            windows += h * w
    print(f"{len(gpu_cases())} cases: worst near-tie share {worst_near}, worst (3 L + 2) A {worst_cond}, changed {changed / pixels:.2f}, "
          f"windows across a guide edge with W < n / 2: {straddle / windows:.2f}")
    assert changed / pixels >= 0.5 and straddle / windows >= 0.1


def conditions(frame, layers, sigmas, radius):
    """(near-tie share, (3 L' + 2) A with L' the layers that are not all zero, or 0 without layers) of one case, by the checker alone;
    asserts that no exponent sits at the cut arg = -126."""
    _, margin, exact = np_median.median(frame, layers, sigmas, radius)
    near = float(((margin <= np_median.DELTA) & ~exact).mean())
    if not layers:
        return near, 0.0
    shape = frame.shape[:2]
    arg = np_median.tap_args(layers, sigmas, radius, shape)
    wt = np_median.tap_weights(layers, sigmas, radius, shape)
    matters = wt > 2.0 ** -24 * wt.sum(-1)[..., None]
    assert not (np.abs(arg + 126.0) < 0.01).any()
    live = sum(1 for l in layers if np.asarray(l)[..., :3].any())
    return near, (3 * live + 2) * (float(np.abs(arg[matters]).max()) if matters.any() else 0.0)


def test_the_other_gpu_cases_meet_the_conditions():
    """The cases of the GPU tests that tests/test_gpu_median.py's uint8 guides do not cover: float16 and float32 guides; the guard-band
    shapes, the planted frames and the strips of test_gpu_median_bounds.py (the strips at 4099 texels, the same recipe); the bands of
    test_gpu_median_huge.py (its two patterns tiled to 80 x 90); the exact constructions, whose exponents are 0 or far below the cut."""
    cases = []
    for gdt in (np.float16, np.float32):
        for radius, n_layers in ((2, 1), (3, 4), (2, 5)):
            noisy, g0, _ = mi.scene(35, 131, seed=35 * 1000 + 131)
            cases.append((f"35x131 {np.dtype(gdt).name} guides", noisy, *mi.layer_set(g0, n_layers, gdt), radius))
    for h, w in ((1, 1), (5, 5), (17, 65), (33, 129), (3, 193)):
        noisy, g0, _ = mi.scene(h, w, seed=h + w)
        for radius in mi.RADII:
            for n_layers, gdt in ((3, np.uint8), (5, np.float16), (1, np.float32)):
                cases.append((f"guard bands {w}x{h}", noisy, *mi.layer_set(g0, n_layers, gdt), radius))
    for where in ("in", "guide", "both"):
        noisy, guide = mi.planted(35, 131, where)
        for radius in mi.RADII:
            cases.append((f"planted {where}", noisy, [guide] + [np.zeros_like(guide)] * 4, [mi.SIGMA0] + [1.0] * 4, radius))
    for shape in ((1, 4099), (4099, 1)):
        frame, guide = mi.strip(*shape)
        cases.append((f"strip {shape}", frame, [guide] + [np.zeros_like(guide)] * 4, [mi.SIGMA0] * 5, 3))
    pat, gpat = mi.huge_patterns()
    ix = np.ix_(np.arange(80) % pat.shape[0], np.arange(90) % pat.shape[1])
    cases.append(("huge bands", pat[ix], [gpat[ix]], [mi.HUGE_SIGMA], 1))
    worst_near, worst_cond = (-1.0, ""), (-1.0, "")
    for name, frame, layers, sigmas, radius in cases:
        near, cond = conditions(frame, layers, sigmas, radius)
        if frame.shape[0] * frame.shape[1] > 1:
            assert near <= mi.NEAR_SHARE, (name, radius, len(layers), near)
        assert cond <= 295, (name, radius, len(layers), cond)
        worst_near, worst_cond = max(worst_near, (near, f"{name} r={radius} L={len(layers)}")), max(worst_cond, (cond, f"{name} r={radius} L={len(layers)}"))
    print(f"{len(cases)} cases: worst near-tie share {worst_near}, worst (3 L' + 2) A {worst_cond}")
    for seed in (1, 2, 3, 9):                                   # the exact constructions: every exponent is 0 or below -7000
        frame, guide = mi.exact_scene(37, 133, seed=seed)
        for radius in mi.RADII:
            arg = np_median.tap_args([guide * np.float32(l + 1) for l in range(16)], [mi.EXACT_SIGMA] * 16, radius, (37, 133))
            inside = np.isfinite(arg)
            assert ((arg[inside] == 0) | (arg[inside] < -7000)).all()


def test_the_demonstration_in_float64():
    """What tests/test_gpu_median_demo.py asserts of the kernels is true of the contract, with twice the margin."""
    noisy, g0, clean = mi.demo()
    r, sigmas = mi.DEMO_RADIUS, [mi.DEMO_SIGMA]
    m_in = mi.mse(noisy, clean)
    m_plain = mi.mse(np_median.median(noisy, None, None, r)[0], clean)
    m_w = mi.mse(np_median.median(noisy, [g0], sigmas, r)[0], clean)
    m_b = mi.mse(np_bilateral_joint.bilateral_joint([noisy], [[g0]], sigmas, 0, r, 2.0)[0], clean)
    print(f"mse: input {m_in:.4g}, plain median {m_plain:.4g}, weighted median {m_w:.4g}, joint bilateral {m_b:.4g}")
    assert 2 * m_plain <= mi.DEMO_PLAIN_RATIO * m_in
    assert 2 * m_w <= mi.DEMO_WEIGHTED_RATIO * m_plain
    assert m_b >= 2 * mi.DEMO_BILATERAL_RATIO * m_w
