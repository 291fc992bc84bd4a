"""GPU suite: mi_denoise with .exr guide layers in the bilateral modes -- FLOAT EXR layers (RGBA32F), and HALF EXR layers with
--half (RGBA16F) -- in --modes layers and --animation --animation-filter layers-temporal: every output file holds the bits of
the Python call on the arrays the files decode to.  Mixed .png / .exr layers and .exr layers in the NLM-layer modes are refused."""
import os
import subprocess

import numpy as np
import pytest

import guide_format_inputs as gi
import image_denoising_filter_amd as mid
from conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "image_denoising_filter_amd", "mi_denoise")
N, SHAPE, R = 3, (45, 133), 8
LAYERS = ("albedo", "normal")                       # (sorted: the order the CLI finds them in)


def _run(cwd, args):
    return subprocess.run([CLI] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=600)


def _make(root, half):
    """EXR frames and, under the discovery naming of the other CLI tests, one FLOAT (or HALF) EXR per frame and layer."""
    d = root / "Animations" / "T"
    (d / "RenderElements").mkdir(parents=True)
    for i, f in enumerate(gi.hdr_frames(SHAPE, N, seed=51)):
        mid.save_image(d / f"Animation01_X_{i:04d}.exr", f)
    rendered = gi.render_layers(SHAPE, N, np.float16 if half else np.float32, seed=52)
    for i in range(N):
        for name, lyr in zip(LAYERS, (rendered[i][1], rendered[i][0])):
            mid.save_image(d / "RenderElements" / f"{name}_{i:04d}.exr", lyr)
    return d


def _decoded(d, half):
    dt = np.float16 if half else np.float32
    as_dt = np.float16 if half else None             # (load_image: None = an .exr as float32)
    frames = [mid.load_image(d / f"Animation01_X_{i:04d}.exr", as_dt) for i in range(N)]
    layers = [[mid.load_image(d / "RenderElements" / f"{name}_{i:04d}.exr", as_dt) for name in LAYERS] for i in range(N)]
    return frames, layers, dt


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 2: np.uint16}[a.dtype.itemsize])


@pytest.mark.parametrize("half", [False, True], ids=["float-layers", "half-layers"])
def test_exr_layers_give_the_python_calls_bits(tmp_path, ctx, half):
    d = _make(tmp_path, half)
    frames, layers, dt = _decoded(d, half)
    assert layers[0][0].dtype == dt and float(np.min(layers[0][1][..., :3])) < -0.5       # signed normals survived the file
    common = ["--gpu-only", "--radius", R, "--sigma-s", gi.SIGMA_S, "--sigma-c", gi.SIGMA_C] + (["--half"] if half else [])
    out = tmp_path / "o"
    out.mkdir()
    r = _run(tmp_path, [d / "Animation01_X_0001.exr", "--modes", "layers", "--outdir", out] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.listdir(out) == ["output-nonlinear-bialteral-layers.exr"]
    want = ctx.bilateral_layers(frames[1], layers[1], R, gi.SIGMA_S, gi.SIGMA_C)
    want = ctx.pack_f16(want) if half else want
    got = mid.load_image(out / "output-nonlinear-bialteral-layers.exr", np.float16 if half else None)
    assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))

    out2 = tmp_path / "o2"
    out2.mkdir()
    r = _run(tmp_path, [d / "Animation01_X_0000.exr", "--animation", "--animation-filter", "layers-temporal", "--temporal-k", 1,
                        "--outdir", out2] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    names = sorted(os.listdir(out2))
    assert names == [f"output-animation-nonlinear-bialteral-layers-multiframe-Animation01_X_{i:04d}.exr" for i in range(N)], names
    want = ctx.bilateral_temporal(frames, 1, radius=R, sigma_s=gi.SIGMA_S, sigma_c=gi.SIGMA_C, layers=layers, out_dtype=dt)
    for i in range(N):
        got = mid.load_image(out2 / names[i], np.float16 if half else None)
        assert got.dtype == want[i].dtype and np.array_equal(_bits(got), _bits(want[i])), i
    # a page-locked budget that admits no frame: the same bytes from pageable frames and layers
    out3 = tmp_path / "o3"
    out3.mkdir()
    r = _run(tmp_path, [d / "Animation01_X_0000.exr", "--animation", "--animation-filter", "layers", "--pinned-mb", 0, "--outdir", out3] + common)
    assert r.returncode == 0, r.stdout + r.stderr
    for i in range(N):
        want_i = ctx.bilateral_layers(frames[i], layers[i], R, gi.SIGMA_S, gi.SIGMA_C)
        got = mid.load_image(out3 / f"output-animation-nonlinear-bialteral-layers-Animation01_X_{i:04d}.exr", np.float16 if half else None)
        assert np.array_equal(_bits(got), _bits(ctx.pack_f16(want_i) if half else want_i)), i


def test_mixed_and_nlm_exr_layers_are_refused(tmp_path):
    d = _make(tmp_path, False)
    u8 = np.full(SHAPE + (4,), 128, np.uint8)
    for mode in (["--modes", "nlm-layers"], ["--animation", "--animation-filter", "nlm-layers"],
                 ["--animation", "--animation-filter", "nlm-layers-temporal"]):
        out = tmp_path / ("n" + str(len(mode)) + mode[-1])
        out.mkdir()
        r = _run(tmp_path, [d / "Animation01_X_0000.exr", "--gpu-only", "--outdir", out] + mode)
        assert r.returncode != 0 and "RGBA8 guide layers only" in r.stdout + r.stderr, r.stdout + r.stderr
        assert os.listdir(out) == []
    os.remove(d / "RenderElements" / "normal_0001.exr")
    mid.save_image(d / "RenderElements" / "normal_0001.png", u8)
    for target, mode in (("Animation01_X_0001.exr", ["--modes", "layers"]),
                         ("Animation01_X_0000.exr", ["--animation", "--animation-filter", "layers-temporal"]),
                         ("Animation01_X_0000.exr", ["--animation", "--animation-filter", "layers"])):
        out = tmp_path / ("m" + str(len(mode)) + mode[-1])
        out.mkdir()
        r = _run(tmp_path, [d / target, "--gpu-only", "--outdir", out] + mode)
        assert r.returncode != 0 and "normal_0001.png" in r.stdout + r.stderr and "one format" in r.stdout + r.stderr, r.stdout + r.stderr
        assert os.listdir(out) == []
